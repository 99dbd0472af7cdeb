"""The opt-in extras of the fused Adam step on the GPU: global-norm gradient clipping and the weight EMA
(optim.FusedAdam / train.Trainer(ema_decay=, ema_warmup=, max_grad_norm=)).

Kernel level (gradients injected through p.grad, no network): norm, p, exp_avg, exp_avg_sq and ema after 5 steps against
the float64 restatement of tests/optim_ref.py.  The tolerance is the project's measured-floor rule: each case computes
e = the float32 restatement's own deviation from float64 on the same inputs and requires the GPU's deviation to be
<= max(4 e, 1e-6), both as max |x - ref| / max |ref| per tensor (optim_ref.rel_err, optim_ref.bound).  Everything else is
bit equality.  Every case prints its figures before it asserts (run with -s); the margins observed on an MI355X are in
profiles/optim_ema_clip.md."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import optim_ref
from conftest import TINY

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 3, 1023, 1024, 1025, 3_000_001)
STEPS = 5
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
B, N, HW = 4, 3, 16


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    params = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    grads = [[((0.5 + s) * 0.01 * rng.standard_normal(n)).astype(np.float32) for n in SIZES] for s in range(STEPS)]
    return params, grads


def _gpu_run(params, grads, lr=1e-3, **opts):
    from view_fusion_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in params]
    opt = FusedAdam(ps, lr=lr, **opts)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g).to(dev)
        opt.step()
        if opt.grad_norm is not None:
            norms.append(opt.grad_norm.clone())
        for p, g in zip(ps, gs):                    # the stored gradient is left unscaled
            assert torch.equal(p.grad.cpu(), torch.from_numpy(g))
    torch.cuda.synchronize()
    sd = opt.state_dict()["state"]
    ema = opt.ema_state_dict()["state"] if opt.ema_decay is not None else None
    return dict(p=[p.detach().cpu().numpy() for p in ps], m=[sd[i]["exp_avg"].cpu().numpy() for i in range(len(ps))],
                v=[sd[i]["exp_avg_sq"].cpu().numpy() for i in range(len(ps))],
                ema=None if ema is None else [ema[i].cpu().numpy() for i in range(len(ps))],
                norm=[float(n) for n in norms], steps=[float(sd[i]["step"]) for i in range(len(ps))])


def _bits_equal(a, b, keys=("p", "m", "v")):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for k in keys for x, y in zip(a[k], b[k]))


CASES = {"clip": dict(clip=True), "ema": dict(ema_decay=0.99), "both": dict(clip=True, ema_decay=0.99),
         "warmup": dict(clip=True, ema_decay=0.99, ema_warmup=True)}


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_match_the_float64_restatement(case):
    params, grads = _inputs()
    kw = dict(CASES[case])
    if kw.pop("clip", False):                       # half the smallest norm of the run: scale < 1 at every step
        kw["max_norm"] = 0.5 * min(optim_ref.run_f64(params, grads)["norm"])
    # the float64 restatement takes the moment betas as the kernels do (float32-rounded: 1 - float32(0.999) is 1.3e-5 off
    # 0.001), so e is the float32 arithmetic's rounding alone and the bound on exp_avg_sq is not loosened by that constant
    r64 = optim_ref.run_f64(params, grads, moment_betas=optim_ref.float_betas(), **kw)
    r32 = optim_ref.run_f32(params, grads, **kw)
    gkw = {("max_grad_norm" if k == "max_norm" else k): v for k, v in kw.items()}
    got = _gpu_run(params, grads, **gkw)
    assert got["steps"] == [float(STEPS)] * len(SIZES)
    if "max_norm" in kw:
        assert all(s < 1.0 for s in r64["scale"])
        for s in range(STEPS):
            e = abs(r32["norm"][s] - r64["norm"][s]) / r64["norm"][s]
            err = abs(got["norm"][s] - r64["norm"][s]) / r64["norm"][s]
            print(f"[{case}] step {s} norm {got['norm'][s]:.9g}: gpu err {err:.3e}  fp32 restatement e {e:.3e}  bound {optim_ref.bound(e):.3e}")
            assert err <= optim_ref.bound(e), (s, err, e)
    else:
        assert got["norm"] == []
    for k in ("p", "m", "v", "ema"):
        if r64[k] is None:
            assert got[k] is None
            continue
        for i, n in enumerate(SIZES):
            e, err = optim_ref.rel_err(r32[k][i], r64[k][i]), optim_ref.rel_err(got[k][i], r64[k][i])
            same = np.array_equal(got[k][i].view(np.uint32), r32[k][i].view(np.uint32))
            print(f"[{case}] {k:3s} numel {n:8d}: gpu err {err:.3e}  fp32 restatement e {e:.3e}  bound {optim_ref.bound(e):.3e}"
                  f"  bit-equal to the fp32 restatement: {same}")
            assert err <= optim_ref.bound(e), (k, n, err, e)


def test_bit_equalities():
    params, grads = _inputs(3)
    plain = _gpu_run(params, grads)
    # a max_grad_norm that never clips: scale == 1 exactly, g * 1 == g
    for big in (1e30, float("inf")):
        loose = _gpu_run(params, grads, max_grad_norm=big)
        assert _bits_equal(plain, loose) and len(loose["norm"]) == STEPS
    # the EMA is a passenger: p, exp_avg, exp_avg_sq do not move by a bit
    ema = _gpu_run(params, grads, ema_decay=0.99, ema_warmup=True)
    assert _bits_equal(plain, ema) and ema["ema"] is not None
    # two identical runs with everything on
    mx = 0.5 * min(optim_ref.run_f64(params, grads)["norm"])
    a = _gpu_run(params, grads, ema_decay=0.99, ema_warmup=True, max_grad_norm=mx)
    b = _gpu_run(params, grads, ema_decay=0.99, ema_warmup=True, max_grad_norm=mx)
    assert _bits_equal(a, b, ("p", "m", "v", "ema")) and a["norm"] == b["norm"]
    assert not _bits_equal(plain, a, ("p",))                      # and the clipping really acted


def _model(dev, sched=SCHED):
    from view_fusion_amd import UNet, ViewFusion
    from view_fusion_amd.utils import deterministic_fill_
    net = UNet(**TINY)
    deterministic_fill_(net.state_dict())
    vf = ViewFusion(net.to(dev), {"train": sched}, True, True)
    vf.set_new_noise_schedule(device=dev, phase="train")
    return vf


def _trainer(dev, graph, **kw):
    from view_fusion_amd import train
    vf = _model(dev)
    tr = train.Trainer(vf, lr_warmup=1, graph=graph, seed=11, **kw)
    tr.it = 0                                      # (lr = peak from the first iteration on)
    return vf, tr


def _batch(dev, s=0):
    from view_fusion_amd import train
    return train.synthetic_batch(B, N, HW, dev, seed=40 + s)


def _snapshot(vf, tr):
    torch.cuda.synchronize()
    sd = tr.opt.state_dict()["state"]
    n = len(list(vf.parameters()))
    out = dict(p=[p.detach().cpu().clone() for p in vf.parameters()], m=[sd[i]["exp_avg"].cpu().clone() for i in range(n)],
               v=[sd[i]["exp_avg_sq"].cpu().clone() for i in range(n)], step=[float(sd[i]["step"]) for i in range(n)])
    if tr.opt.ema_decay is not None:
        ema = tr.ema_state_dict()
        out["ema"] = [ema["state"][i].cpu().clone() for i in range(n)]
        out["ema_t"] = ema["num_updates"]
    return out


def _same(a, b):
    return all(a[k] == b[k] if k in ("step", "ema_t") else all(torch.equal(x, y) for x, y in zip(a[k], b[k])) for k in a)


def _max_norm(dev):
    """Half the gradient norm of the first iteration of the plain run (an eager step, its p.grad summed in double)."""
    vf, tr = _trainer(dev, False)
    tr.step(_batch(dev))
    return 0.5 * float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in vf.parameters())))


def test_defaults_launch_the_old_entry_points_and_keep_the_state_dict():
    from view_fusion_amd import ops
    from view_fusion_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    ps = [torch.nn.Parameter(torch.randn(n, device=dev)) for n in (5, 2000)]
    opt = FusedAdam(ps)
    vf, tr = _trainer(dev, None)
    ops.st.KERNEL_LOG = []
    try:
        for p in ps:
            p.grad = torch.randn_like(p)
        opt.step()
        names = [r[5] for r in ops.st.KERNEL_LOG]
        assert names == ["vf_adam_multi"], names
        del ops.st.KERNEL_LOG[:]
        tr.step(_batch(dev))
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    opt_names = [n for n in names if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))]
    assert opt_names == ["vf_adam_multi"], opt_names
    assert opt.grad_norm is None and tr.grad_norm is None
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
    assert set(sd["param_groups"][0]) <= set(ref)
    # and with the extras on, the new ones
    opt2 = FusedAdam(ps, ema_decay=0.9, max_grad_norm=1.0)
    ops.st.KERNEL_LOG = []
    try:
        opt2.step()
        names = [r[5] for r in ops.st.KERNEL_LOG]
    finally:
        ops.st.KERNEL_LOG = None
    assert names == ["vf_adam_set_scalars_ex", "vf_grad_sumsq_multi", "vf_grad_norm_finish", "vf_adam_multi_ex"], names
    assert set(opt2.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


def test_defaults_capture_and_replay_through_the_old_entry_points(monkeypatch):
    """Options off, the iteration as a graph: the capture holds vf_adam_multi_dev, every replay is preceded by
    vf_adam_set_scalars, and none of the new entry points is reached (these calls bypass the kernel log)."""
    from view_fusion_amd import _lib, train
    dev = torch.device("cuda:0")
    names, real = [], _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    vf, tr = _trainer(dev, True)
    for s in range(5):
        tr.step(_batch(dev, s))
    torch.cuda.synchronize()
    replays = 5 - train.Trainer.GRAPH_AFTER
    assert tr.mode == "graph" and tr.graph_steps == replays
    opt_names = [n for n in names if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))]
    assert opt_names == ["vf_adam_multi"] * train.Trainer.GRAPH_AFTER + ["vf_adam_multi_dev"] + ["vf_adam_set_scalars"] * replays, opt_names
    # and with the options on, the new ones in their place
    del names[:]
    vf, tr = _trainer(dev, True, ema_decay=0.9, max_grad_norm=1.0)
    for s in range(4):
        tr.step(_batch(dev, s))
    torch.cuda.synchronize()
    opt_names = [n for n in names if n.startswith(("vf_adam", "vf_grad_", "vf_swap"))]
    eager = ["vf_adam_set_scalars_ex", "vf_grad_sumsq_multi", "vf_grad_norm_finish", "vf_adam_multi_ex"]
    assert opt_names == eager * 2 + ["vf_grad_sumsq_multi", "vf_grad_norm_finish", "vf_adam_multi_ex_dev"] + \
        ["vf_adam_set_scalars_ex"] * 2, opt_names
    with pytest.raises(ValueError):
        tr.opt.max_grad_norm = None                # (the norm launches are part of what was captured)
    with pytest.raises(ValueError):
        train.Trainer(_model(dev)).opt.max_grad_norm = 1.0


def test_trainer_graph_replay_equals_eager_and_reports_the_norm():
    dev = torch.device("cuda:0")
    kw = dict(ema_decay=0.9, ema_warmup=True, max_grad_norm=_max_norm(dev))
    (vf_e, tr_e), (vf_g, tr_g) = _trainer(dev, False, **kw), _trainer(dev, True, **kw)
    first = None
    for s in range(6):
        tr_e.step(_batch(dev, s))
        tr_g.step(_batch(dev, s))
        torch.cuda.synchronize()
        assert float(tr_e.grad_norm) == float(tr_g.grad_norm), s
        first = float(tr_g.grad_norm) if first is None else first
    from view_fusion_amd import train
    assert tr_g.mode == "graph" and tr_g.graph_steps == 6 - train.Trainer.GRAPH_AFTER and tr_e.graph_steps == 0
    a, b = _snapshot(vf_e, tr_e), _snapshot(vf_g, tr_g)
    assert _same(a, b) and a["ema_t"] == 6 and a["step"][0] == 6.0
    # the norm the replayed step reports vs the gradients of the eager run of the same step, summed in double
    gs = [p.grad.detach().cpu().numpy() for p in vf_e.parameters()]
    ref = float(np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs)))
    e = abs(float(optim_ref.norm_scale_f32(gs, None)[0]) - ref) / ref
    err = abs(float(tr_g.grad_norm) - ref) / ref
    print(f"trainer grad_norm {float(tr_g.grad_norm):.9g}: err {err:.3e}  fp32 restatement e {e:.3e}  max_grad_norm {kw['max_grad_norm']:.4g}")
    assert err <= optim_ref.bound(e)
    assert first > kw["max_grad_norm"]                             # clipping was active (twice max_norm at iteration 0)
    # the captured step reads max_norm from device memory: changing it needs no new capture
    tr_e.opt.max_grad_norm = tr_g.opt.max_grad_norm = 0.25 * kw["max_grad_norm"]
    steps = tr_g.graph_steps
    tr_e.step(_batch(dev, 6))
    tr_g.step(_batch(dev, 6))
    assert tr_g.graph_steps == steps + 1 and _same(_snapshot(vf_e, tr_e), _snapshot(vf_g, tr_g))


def test_ema_weights_exchange():
    dev = torch.device("cuda:0")
    kw = dict(ema_decay=0.9, max_grad_norm=_max_norm(dev))
    (vf_a, tr_a), (vf_b, tr_b) = _trainer(dev, True, **kw), _trainer(dev, True, **kw)
    for s in range(3):
        tr_a.step(_batch(dev, s))
        tr_b.step(_batch(dev, s))
    before = _snapshot(vf_a, tr_a)
    assert any(not torch.equal(p, e) for p, e in zip(before["p"], before["ema"]))
    g = torch.Generator().manual_seed(5)
    cond, angle, vc = torch.rand(2, N, 3, HW, HW, generator=g).to(dev), torch.rand(2, 1, generator=g).to(dev), torch.tensor([3, 2])
    with torch.no_grad():
        live = vf_a(y_cond=cond, view_count=vc, angle=angle, generate=True, seed=9)[1].clone()   # (packs the live weights)
        with tr_a.ema_weights() as m:
            assert m is vf_a
            for p, e in zip(vf_a.parameters(), before["ema"]):
                assert torch.equal(p.detach().cpu(), e)
            inside = vf_a(y_cond=cond, view_count=vc, angle=angle, generate=True, seed=9)[1].clone()
        fresh = _model(dev)
        for p, e in zip(fresh.parameters(), before["ema"]):
            p.copy_(e.to(dev))
        want = fresh(y_cond=cond, view_count=vc, angle=angle, generate=True, seed=9)[1]
    assert torch.equal(inside, want) and not torch.equal(inside, live)
    assert _same(before, _snapshot(vf_a, tr_a))
    tr_a.step(_batch(dev, 3))
    tr_b.step(_batch(dev, 3))
    assert tr_a.graph_steps == tr_b.graph_steps == 2
    assert _same(_snapshot(vf_a, tr_a), _snapshot(vf_b, tr_b))


def test_checkpoint_round_trip(tmp_path):
    from view_fusion_amd import drivers
    dev = torch.device("cuda:0")
    kw = dict(ema_decay=0.9, ema_warmup=True, max_grad_norm=_max_norm(dev))
    vf_u, tr_u = _trainer(dev, False, **kw)
    for s in range(5):
        tr_u.step(_batch(dev, s))
    vf_a, tr_a = _trainer(dev, False, **kw)
    for s in range(3):
        tr_a.step(_batch(dev, s))
    path = str(tmp_path / "ckpt.pt")
    drivers.save_checkpoint(path, vf_a, tr_a.opt, ema=tr_a.ema_state_dict(), it=tr_a.it)
    vf_c, tr_c = _trainer(dev, False, **kw)
    rest = drivers.load_checkpoint(path, vf_c, tr_c.opt, device=dev)
    assert set(rest) == {"ema", "it"} and rest["ema"]["num_updates"] == 3
    tr_c.it = rest["it"]
    assert _same(_snapshot(vf_a, tr_a), _snapshot(vf_c, tr_c))
    for s in range(3, 5):
        tr_c.step(_batch(dev, s))
    assert _same(_snapshot(vf_u, tr_u), _snapshot(vf_c, tr_c))
    # an optimizer checkpoint still interchanges with torch.optim.Adam
    ref = torch.optim.Adam(list(vf_c.parameters()), lr=1e-4)
    ref.load_state_dict(tr_c.opt.state_dict())


def _worker(rank, world, port, out, max_norm, steps):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      VF_REDUCER="arena")
    import torch.distributed as dist
    from view_fusion_amd import train
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vf = _model(dev)
    tr = train.Trainer(vf, world=world, lr_warmup=1, graph=False, seed=11, ema_decay=0.9, ema_warmup=True,
                       max_grad_norm=max_norm)
    tr.it = 0
    norms = []
    for s in range(steps):
        tr.step(train.synthetic_batch(B, N, HW, dev, seed=70 + 10 * s + rank))
        norms.append(float(tr.grad_norm))
    snap = _snapshot(vf, tr)
    out[rank] = dict(p=snap["p"], ema=snap["ema"], norms=norms, reducer=tr.dist_info()["reducer"])
    dist.barrier()
    dist.destroy_process_group()


def _spawn(max_norm, steps=4):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out, max_norm, steps), nprocs=2, join=True)
    return out[0], out[1]


def test_two_ranks_stay_identical():
    """Two processes sharing the GPU, the default reducer (gradient arena over gloo), both extras on: the norm is taken
    on the averaged gradients, so both ranks clip alike."""
    r0, r1 = _spawn(float("inf"))                   # measures the norms, never clips
    assert r0["norms"] == r1["norms"] and r0["reducer"] == "arena"
    mx = 0.5 * min(r0["norms"])
    r0, r1 = _spawn(mx)
    assert r0["norms"] == r1["norms"] and r0["norms"][0] > mx     # (the first norm is that of the measuring run)
    for k in ("p", "ema"):
        for a, b in zip(r0[k], r1[k]):
            assert torch.equal(a, b), k
    assert any(not torch.equal(a, b) for a, b in zip(r0["p"], r0["ema"]))


def test_xgmi_reducer_with_the_extras_is_refused(monkeypatch):
    from view_fusion_amd import train
    vf = _model(torch.device("cuda:0"))
    monkeypatch.setenv("VF_REDUCER", "xgmi")
    for kw in (dict(ema_decay=0.99), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="xgmi"):
            train.Trainer(vf, **kw)
    train.Trainer(vf)                               # (without them the variable alone changes nothing at world 1)
