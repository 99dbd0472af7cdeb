"""tools/loss_bits.py's compare logic on synthetic JSON (no GPU): equal runs, a changed digest, a case on one side only;
the same on the keys of the hybrid-loss and stacking grids, whose cases carry other digest names."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("loss_bits", os.path.join(ROOT, "tools", "loss_bits.py"))
lb = importlib.util.module_from_spec(spec)
spec.loader.exec_module(lb)

RUN = {"8x8/eps/mse/None/scale0/w1/hist0": dict(loss="aa", sample_loss="bb", weight="cc", grad="dd", bin_sum=None,
                                                  bin_cnt=None),
       "8x8/v/l1/p2/scale1/w0/hist1": dict(loss="ab", sample_loss="bc", weight="cd", grad="de", bin_sum="ef", bin_cnt="f0"),
       "8x8/compose_mse_loss/w1": dict(loss="01", grad="02")}


def write(tmp_path, name, digests):
    p = tmp_path / name
    p.write_text(json.dumps(dict(cases=len(digests), digests=digests)))
    return str(p)


def test_compare_finds_a_changed_digest_and_a_missing_case(tmp_path, capsys):
    assert lb.compare(RUN, json.loads(json.dumps(RUN))) == []
    changed = json.loads(json.dumps(RUN))
    changed["8x8/v/l1/p2/scale1/w0/hist1"]["grad"] = "00"
    assert lb.compare(changed, RUN) == ["8x8/v/l1/p2/scale1/w0/hist1"]
    fewer = {k: v for k, v in RUN.items() if "compose_mse_loss" not in k}
    assert lb.compare(fewer, RUN) == lb.compare(RUN, fewer) == ["8x8/compose_mse_loss/w1"]

    old = write(tmp_path, "old.json", RUN)
    assert lb.main(["--compare", old, write(tmp_path, "same.json", RUN)]) == 0
    assert "0 of 3 cases differ" in capsys.readouterr().out
    assert lb.main(["--compare", old, write(tmp_path, "changed.json", changed)]) == 1
    out = capsys.readouterr().out
    assert "1 of 3 cases differ" in out and "'grad': '!='" in out and "'loss': '='" in out


RUN_LV = {"12x20/vlb/v/huber/lam0.001/w1/hist1": dict(loss="aa", sample_loss="bb", weight="cc", sample_vlb="dd", grad="ee",
                                                     bin_sum="ff", bin_cnt="00"),
          "12x20/vlb/eps/mse/lam0.0/w0/hist0": dict(loss="ab", sample_loss="bc", weight="cd", sample_vlb="de", grad="ef",
                                                   bin_sum=None, bin_cnt=None),
          "8x8/stack/cc6/drop1/null1/sc_given/noise0/copy0": dict(x="11", level_s="22", angle_s="33"),
          "8x8/stack/cc3/drop0/null0/sc_none/noise1/copy1": dict(x="12", level_s="23", angle_s="34")}


def test_compare_on_the_hybrid_loss_and_stacking_keys(tmp_path, capsys):
    assert lb.compare(RUN_LV, json.loads(json.dumps(RUN_LV))) == []
    changed = json.loads(json.dumps(RUN_LV))
    changed["12x20/vlb/v/huber/lam0.001/w1/hist1"]["sample_vlb"] = "0d"
    changed["8x8/stack/cc6/drop1/null1/sc_given/noise0/copy0"]["x"] = "10"
    assert lb.compare(changed, RUN_LV) == ["12x20/vlb/v/huber/lam0.001/w1/hist1",
                                           "8x8/stack/cc6/drop1/null1/sc_given/noise0/copy0"]
    fewer = {k: v for k, v in RUN_LV.items() if "/stack/" not in k}
    assert lb.compare(fewer, RUN_LV) == lb.compare(RUN_LV, fewer) == sorted(k for k in RUN_LV if "/stack/" in k)

    old = write(tmp_path, "old.json", RUN_LV)
    assert lb.main(["--compare", old, write(tmp_path, "same.json", RUN_LV)]) == 0
    assert "0 of 4 cases differ" in capsys.readouterr().out
    assert lb.main(["--compare", old, write(tmp_path, "changed.json", changed)]) == 1
    out = capsys.readouterr().out
    assert "2 of 4 cases differ" in out and "'sample_vlb': '!='" in out and "'x': '!='" in out and "'angle_s': '='" in out
