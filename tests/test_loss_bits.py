"""tools/loss_bits.py's compare logic on synthetic JSON (no GPU): equal runs, a changed digest, a case on one side only."""
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
