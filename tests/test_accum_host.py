"""CPU checks of gradient accumulation's host side (train.Trainer(accum_steps=), train.split_batch) and of the numpy
restatement tests/accum_ref.py that the GPU tests compare the accumulate launch with, bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import accum_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StandIn(torch.nn.Module):
    """ViewFusion.forward's signature on the CPU (the HIP model has no CPU path)."""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Conv2d(3, 3, 3, padding=1)

    def forward(self, y_cond, view_count, angle, y_0=None, noise=None, generate=False):
        return torch.nn.functional.mse_loss(self.net(y_cond.mean(dim=1)), y_0)


# ---- the restatement ---------------------------------------------------------------------------------------------
def test_restatement_rounds_each_operation_to_float32():
    rng = np.random.default_rng(0)
    g = rng.standard_normal(4099).astype(np.float32)
    acc = rng.standard_normal(4099).astype(np.float32)
    w = np.float32(1.0 / 3.0)
    got = accum_ref.accumulate(acc, g, 1.0, 1.0 / 3.0)
    assert got.dtype == np.float32
    # product of two floats is exact in double: rounding it to float is THE float32 product; the float32 sum of two
    # floats of similar magnitude equals the double sum rounded once (the double sum is exact here)
    prod = (np.float64(w) * g.astype(np.float64)).astype(np.float32)
    want = (acc.astype(np.float64) + prod.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and it is NOT the fused multiply-add (one rounding) everywhere: the convention is observable
    fused = (np.float64(w) * g.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(got.view(np.uint32), fused.view(np.uint32))


def test_restatement_first_launch_does_not_read_the_accumulator():
    g = np.array([1.5, -0.0, 3.0, 1e-30], dtype=np.float32)
    nan = np.full(4, np.nan, dtype=np.float32)
    got = accum_ref.accumulate(nan, g, 0.0, 0.5)
    assert np.array_equal(got.view(np.uint32), (np.float32(0.5) * g).view(np.uint32))
    assert np.signbit(got[1])                                      # w g alone: -0 stays -0 (0 * acc + w g would not)
    assert np.all(np.isnan(accum_ref.accumulate(nan, g, 1.0, 0.5)))


def test_accumulate_all_is_the_weighted_sum():
    rng = np.random.default_rng(1)
    micro = [[rng.standard_normal(n).astype(np.float32) for n in (1, 5, 1025)] for _ in range(4)]
    acc = accum_ref.accumulate_all(micro, [0.25] * 4)
    for i, a in enumerate(acc):
        want = sum(0.25 * m[i].astype(np.float64) for m in micro)
        assert np.abs(a - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max() + 1e-12
    # weights that are powers of two on equal micro-gradients: exact
    same = accum_ref.accumulate_all([micro[0], micro[0]], [0.5, 0.5])
    assert all(np.array_equal(a, g) for a, g in zip(same, micro[0]))


# ---- the splitter and the id arithmetic ------------------------------------------------------------------------------
@pytest.mark.parametrize("it,B,A", [(0, 4, 2), (7, 4, 4), (3, 6, 3), (2 ** 20, 16, 4), (5, 12, 1), (1, 160, 8)])
def test_micro_batch_ids_are_the_full_batch_ids(it, B, A):
    from view_fusion_amd import train
    first = train.step_sample_ids(it, B)
    ids = torch.arange(B, dtype=torch.int64) + first
    batch = train.synthetic_batch(B, 3, 8, "cpu", seed=it % 100, ragged=True)
    parts = train.split_batch(batch, dict(seed=5, sample_ids=ids), A)
    assert len(parts) == A
    n = B // A
    for m, (bm, em) in enumerate(parts):
        assert em["seed"] == 5
        assert torch.equal(em["sample_ids"], first + m * n + torch.arange(n))      # the issue's formula
        assert bm["y_0"].shape[0] == n
    assert torch.equal(torch.cat([em["sample_ids"] for _, em in parts]), ids)
    for k in ("y_0", "y_cond", "angle", "view_count"):
        assert torch.equal(torch.cat([bm[k] for bm, _ in parts]), batch[k]), k
    # ids never repeat across iterations either
    assert train.step_sample_ids(it + 1, B) == first + B


def test_split_batch_cuts_every_per_sample_input():
    from view_fusion_amd import train
    B, hw = 4, 8
    batch = train.synthetic_batch(B, 3, hw, "cpu", seed=0)
    batch["view_count"] = [1, 3, 2, 2]                              # a list
    g = torch.Generator().manual_seed(1)
    extra = dict(t=torch.randint(1, 10, (B,), generator=g), u=torch.rand(B, 1, generator=g),
                 noise=torch.randn(B, 3, hw, hw, generator=g), sample_ids=[10, 11, 12, 13], seed=3, y_t=None)
    parts = train.split_batch(batch, extra, 2)
    assert [bm["view_count"] for bm, _ in parts] == [[1, 3], [2, 2]]
    assert [em["sample_ids"] for _, em in parts] == [[10, 11], [12, 13]]
    for k in ("t", "u", "noise"):
        assert torch.equal(torch.cat([em[k] for _, em in parts]), extra[k])
        assert parts[1][1][k].data_ptr() != extra[k].data_ptr() and parts[0][1][k].data_ptr() == extra[k].data_ptr()  # views
    assert all(em["seed"] == 3 and em["y_t"] is None for _, em in parts)
    one = train.split_batch(batch, extra, 1)
    assert len(one) == 1 and torch.equal(one[0][0]["y_0"], batch["y_0"]) and one[0][0]["view_count"] == [1, 3, 2, 2]


@pytest.mark.parametrize("B,A", [(4, 3), (5, 2), (2, 4), (4, 0)])
def test_split_batch_refuses_a_batch_the_steps_do_not_divide(B, A):
    from view_fusion_amd import train
    with pytest.raises(ValueError, match="accum_steps"):
        train.split_batch(train.synthetic_batch(B, 2, 8, "cpu"), {}, A)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_trainer_refuses_accumulation_on_a_cpu_model_and_across_ranks(monkeypatch):
    from view_fusion_amd import train
    with pytest.raises(ValueError, match="GPU"):
        train.Trainer(StandIn(), accum_steps=2)
    for kind in ("arena", "ddp", "xgmi"):
        monkeypatch.setenv("VF_REDUCER", kind)
        with pytest.raises(ValueError, match="single-process"):
            train.Trainer(StandIn(), world=2, accum_steps=2)
    monkeypatch.delenv("VF_REDUCER")
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="accum_steps"):
            train.Trainer(StandIn(), accum_steps=bad)
    tr = train.Trainer(StandIn(), accum_steps=1)                    # the default, spelled out: today's trainer
    assert tr.accum_steps == 1 and train.Trainer(StandIn()).accum_steps == 1
    loss = tr.step(train.synthetic_batch(4, 3, 8, "cpu"))
    assert torch.isfinite(loss)


def test_c_abi_declares_the_accumulate_launch():
    from view_fusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    m = re.search(r"int vf_grad_accum_multi\(([^)]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["vf_grad_accum_multi"]) == 5
