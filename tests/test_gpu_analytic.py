"""The moment kernel of the analytic variance on the GPU, through the C ABI (ops.eps_moments; eps_moment_kernel and the
bound's nll_finish_kernel of csrc/diffusion.hip; definition at the head of that file) against the float64 restatement
tests/analytic_ref.py.

  1. eps / v / x0 x softmax / mean x six- and nine-channel outputs, B = 3 with ragged view counts (1, 3, 2), a step of
     its own per sample and one of them out of range (clamped into the chain), at the smallest shapes at which this
     geometry can go wrong -- 2x2 (3 float4: one partial wave), 8x8 (fewer float4 than one workgroup), 12x20 (a channel
     boundary inside a chunk, HW % 256 != 0), 32x32 (several chunks).
     Tolerance: no number fixed in advance.  The float32 run of the restatement on the same inputs measures the formulas'
     own rounding floor against the float64 run; the maximum of that over the cases, times 4, is what the device gets (it
     reduces 256-wide in another order).  Only column k of a sample's row is written; the nine-channel run gives the
     six-channel run's bits (channels 6..8 are never read).
  2. 128x192 at B = 1: every thread takes a second trip and all 64 partials are in use.
  3. the same bits on two runs, and for B = 3 against the same samples one at a time and in another order.
Figures are printed before the assertions (run with -s); profiles/analytic_variance.md records them."""
import numpy as np
import pytest
import torch

import analytic_ref

pytestmark = pytest.mark.gpu
SCHED = dict(schedule="linear", num_timesteps=20, linear_start=1e-4, linear_end=0.09)
T = SCHED["num_timesteps"]
VC = (1, 3, 2)
SHAPES = [(2, 2), (8, 8), (12, 20), (32, 32)]
PREDS = ("eps", "v", "x0")
KIDX = {(2, 2): (5, 0, T + 5), (8, 8): (-3, 12, 7), (12, 20): (T - 1, 1, 2 * T), (32, 32): (9, T + 1, 3)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


_TABS, _CASES = {}, {}


def _tabs(prediction):
    """The fp32 table values the device reads, on the host."""
    if prediction not in _TABS:
        from view_fusion_amd import schedule
        betas = schedule.make_beta_schedule(**SCHED)
        _TABS[prediction] = {k: v.astype(np.float32) for k, v in schedule.eps_tables(betas, None, prediction).items()}
    return _TABS[prediction]


def _case(hw, vc, seed=21):
    """Fixed-seed inputs, built once and left unchanged: a nine-channel output (its first six channels are the six-channel
    case) and the noisy targets."""
    key = (tuple(hw), tuple(vc), seed)
    if key not in _CASES:
        g = np.random.default_rng(seed + hw[0])
        out = g.standard_normal((sum(vc), 9) + tuple(hw)).astype(np.float32)
        out[:, 3:6] *= 2.0
        _CASES[key] = dict(out=out, y_k=(1.3 * g.standard_normal((len(vc), 3) + tuple(hw))).astype(np.float32))
    return _CASES[key]


def _dv(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run(dev, tab, case, ks, vc, weighting, channels=6, rows=None):
    """ops.eps_moments on one case (rows: the samples to run, default all) -> float32 (B,), the sample's own column."""
    from view_fusion_amd import ops
    rows = list(range(len(vc))) if rows is None else rows
    off_h = np.concatenate([[0], np.cumsum(vc)])
    views = np.concatenate([np.arange(off_h[i], off_h[i + 1]) for i in rows])
    off, _, _ = ops.view_offsets([vc[i] for i in rows], dev)
    tabs = {n: _dv(dev, tab[n]) for n in ("ea", "eb")}
    kidx = torch.tensor([ks[i] for i in rows], device=dev, dtype=torch.int64)
    m2 = ops.eps_moments(_dv(dev, case["out"][views][:, :channels]), off, _dv(dev, case["y_k"][rows]), kidx, tabs,
                         len(rows), weighting)
    assert tuple(m2.shape) == (len(rows), T)
    cols = [min(max(ks[i], 0), T - 1) for i in rows]
    mask = torch.ones_like(m2, dtype=torch.bool)
    mask[torch.arange(len(rows)), torch.tensor(cols)] = False
    assert not m2[mask].any()                                        # only column k of each row is written
    return m2[torch.arange(len(rows)), torch.tensor(cols)].cpu().numpy()


def _refs(tab, case, ks, vc, weighting):
    cols = [min(max(k, 0), T - 1) for k in ks]
    ea, eb = tab["ea"][cols], tab["eb"][cols]
    args = (case["out"], vc, weighting, case["y_k"], ea, eb)
    return analytic_ref.moment(*args, dt=np.float64), analytic_ref.moment(*args, dt=np.float32)


# ---- 1. the kernel against float64 ---------------------------------------------------------------------------------------------
def test_moments_against_float64(dev):
    rec = []
    for prediction in PREDS:
        tab = _tabs(prediction)
        for weighting in (True, False):
            for hw in SHAPES:
                n4 = 3 * hw[0] * hw[1] // 4
                assert {(2, 2): n4 == 3, (8, 8): n4 < 256, (12, 20): n4 % 256 != 0 and (hw[0] * hw[1]) % 256 != 0,
                        (32, 32): n4 > 2 * 256}[hw]
                case, ks = _case(hw, VC), KIDX[hw]
                r64, r32 = _refs(tab, case, ks, VC, weighting)
                six = _run(dev, tab, case, ks, VC, weighting, 6)
                nine = _run(dev, tab, case, ks, VC, weighting, 9)
                assert np.array_equal(six, nine), (prediction, weighting, hw)        # channels 6..8 are never read
                if not weighting:                                                    # the mean reads channels 0..2 alone
                    assert np.array_equal(six, _run(dev, tab, case, ks, VC, weighting, 3))
                e32 = float((np.abs(r32.astype(np.float64) - r64) / r64).max())
                e = float((np.abs(six.astype(np.float64) - r64) / r64).max())
                rec.append((prediction, weighting, hw, e, e32))
    floor = max(r[4] for r in rec)
    tol = 4.0 * floor
    worst = max(rec, key=lambda r: r[3])
    print(f"eps_moment_kernel: {len(rec)} cases x 6 / 9 channels, fp32 restatement floor {floor:.2e}, tolerance {tol:.2e}, "
          f"device worst {worst[3]:.2e} at {worst[:3]}")
    assert floor > 0
    bad = [r for r in rec if not r[3] <= tol]
    assert not bad, bad


def test_eps_prediction_is_the_plain_second_moment(dev):
    """eps: ea = 0, eb = 1, so the level does not matter and the moment is that of the composed output itself."""
    tab, case = _tabs("eps"), _case((12, 20), VC)
    a = _run(dev, tab, case, (0, 7, T - 1), VC, True)
    b = _run(dev, tab, case, (T - 1, 2, 4), VC, True)
    assert np.array_equal(a, b)


# ---- 2. the grid-stride trip -----------------------------------------------------------------------------------------------------
def test_grid_stride_loop(dev):
    """128x192 at B = 1: 3 HW / 4 = 18432 float4 > 64 workgroups x 256, so every thread takes a second trip and all 64
    partials are in use (the other shapes never stride)."""
    rec = []
    for prediction, weighting, channels in (("v", True, 6), ("x0", False, 9)):
        tab, case = _tabs(prediction), _case((128, 192), (2,))
        r64, r32 = _refs(tab, case, (7,), (2,), weighting)
        got = _run(dev, tab, case, (7,), (2,), weighting, channels)
        e32, e = float(abs(float(r32[0]) - r64[0]) / r64[0]), float(abs(float(got[0]) - r64[0]) / r64[0])
        print(f"128x192 {prediction} weighting {weighting} {channels} channels: device {e:.2e}  fp32 restatement {e32:.2e}")
        rec.append((e, e32))
    floor = max(r[1] for r in rec)
    assert floor > 0 and all(r[0] <= 4.0 * floor for r in rec), rec


# ---- 3. the same bits on every run and for every batch -------------------------------------------------------------------------
@pytest.mark.parametrize("prediction,weighting", [("v", True), ("x0", False)])
def test_bits_do_not_depend_on_the_run_or_the_batch(dev, prediction, weighting):
    tab = _tabs(prediction)
    for hw in ((12, 20), (32, 32)):
        case, ks = _case(hw, VC), KIDX[hw]
        one = _run(dev, tab, case, ks, VC, weighting)
        two = _run(dev, tab, case, ks, VC, weighting)
        assert np.array_equal(one, two)
        for i in range(len(VC)):
            alone = _run(dev, tab, case, ks, VC, weighting, rows=[i])
            assert alone[0] == one[i], (hw, i)
        back = _run(dev, tab, case, ks, VC, weighting, rows=[2, 0, 1])
        assert np.array_equal(back, one[[2, 0, 1]])


def test_preallocated_outputs_and_argument_checks(dev):
    from view_fusion_amd import _lib, ops
    tab, case = _tabs("v"), _case((8, 8), VC)
    off, _, _ = ops.view_offsets(VC, dev)
    tabs = {n: _dv(dev, tab[n]) for n in ("ea", "eb")}
    out, y_k = _dv(dev, case["out"][:, :6]), _dv(dev, case["y_k"])
    kidx = torch.tensor([1, 2, 3], device=dev, dtype=torch.int64)
    m2 = torch.full((3, T), -1.0, device=dev)
    scratch = ops.nll_scratch(3, dev)
    got = ops.eps_moments(out, off, y_k, kidx, tabs, 3, True, out=m2, scratch=scratch)
    assert got is m2 and int((m2 == -1.0).sum()) == 3 * T - 3         # three columns written, nothing else touched
    fresh = ops.eps_moments(out, off, y_k, kidx, tabs, 3, True)
    assert torch.equal(fresh[[0, 1, 2], [1, 2, 3]], m2[[0, 1, 2], [1, 2, 3]])
    for bad in (dict(out=torch.zeros(3, T - 1, device=dev)), dict(scratch={"vb": torch.zeros(8, device=dev)})):
        with pytest.raises(ValueError):
            ops.eps_moments(out, off, y_k, kidx, tabs, 3, True, **bad)
    with pytest.raises(ValueError):
        ops.eps_moments(out, off, y_k[:2].contiguous(), kidx, tabs, 3, True)
    with pytest.raises(_lib.VFHipError):
        ops.eps_moments(out, off, y_k, kidx.int(), tabs, 3, True)
    with pytest.raises(_lib.VFHipError):                              # the softmax needs the logit channels
        ops.eps_moments(out[:, :3].contiguous(), off, y_k, kidx, tabs, 3, True)
