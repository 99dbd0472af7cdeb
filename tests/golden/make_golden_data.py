"""Writes tests/golden/data_plan.npz: what the reference loader's process_sample (data/nmr_dataset.py) does to the 24
views of an object, recorded as view indices.  Run once, with the reference checkout on the path:

    python tests/golden/make_golden_data.py /path/to/reference

For numpy seeds 0..199 x {train, test} it runs process_sample on 24 tiny 2 x 2 images whose pixels encode (view,
channel, position), and records -- replayed from the same numpy seed -- p (images_idx after the first shuffle), the
coin, q (images_idx at the end) and the view indices that target / cond / relative_cond (both halves) show, plus both
angles as float32.  Only this data is committed; nothing of the reference's code is."""
import os
import sys
import types

import numpy as np

SEEDS, MODES = range(200), ("train", "test")


def encoded(view):
    """(2, 2, 3) HWC float32: pixel = 10 * view + 4 * channel + position, all distinct and < 256."""
    img = np.zeros((2, 2, 3), dtype=np.float32)
    for c in range(3):
        for pos in range(4):
            img[pos // 2, pos % 2, c] = 10 * view + 4 * c + pos
    return img


def view_of(chw):
    """The view an output image (3, 2, 2) shows; checks every pixel."""
    v = int(chw[0, 0, 0]) // 10
    assert np.array_equal(chw, encoded(v).transpose(2, 0, 1)), "an output image is not one of the inputs"
    return v


def main(ref):
    sys.path.insert(0, ref)
    sys.modules.setdefault("webdataset", types.ModuleType("webdataset"))      # not used by process_sample
    from data.nmr_dataset import process_sample
    sample = {f"{i:04d}.png": encoded(i) for i in range(24)}
    sample["__key__"] = "obj"
    rec = {k: [] for k in ("seed", "train", "p", "coin", "q", "target", "cond", "rel_ref", "rel_cond", "angle",
                           "relative_angle")}
    for mode in MODES:
        for s in SEEDS:
            np.random.seed(s)
            out = process_sample(sample, mode=mode)
            np.random.seed(s)                                     # replay the draws
            idx = np.arange(24)
            np.random.shuffle(idx)
            p = idx.copy()
            coin = np.random.random()
            if coin < 0.1 and mode == "train":
                np.random.shuffle(idx)
            rec["seed"].append(s)
            rec["train"].append(mode == "train")
            rec["p"].append(p)
            rec["coin"].append(coin)
            rec["q"].append(idx.copy())
            rec["target"].append(view_of(out["target"]))
            rec["cond"].append([view_of(v) for v in out["cond"]])
            rec["rel_ref"].append([view_of(v[:3]) for v in out["relative_cond"]])
            rec["rel_cond"].append([view_of(v[3:]) for v in out["relative_cond"]])
            assert out["angle"].dtype == out["relative_angle"].dtype == np.float32
            rec["angle"].append(out["angle"][0])
            rec["relative_angle"].append(out["relative_angle"][0])
            assert [view_of(v) for v in out["all_views"]] == list(range(24))
    arrays = {k: np.asarray(v) for k, v in rec.items()}
    taken = int(((arrays["coin"] < 0.1) & arrays["train"]).sum())
    print(f"{len(arrays['seed'])} cases, {taken} take the second shuffle")
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data_plan.npz")
    np.savez_compressed(dst, **arrays)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
