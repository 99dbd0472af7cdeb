"""tools/kernel_isa_diff.py on two small synthetic listings: each of its three verdicts, and --map."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
kid = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kid)


def listing(kernels):
    """kernels: [(symbol, function number, body lines, kernarg size)] -> the text of a listing as hipcc -S lays it out"""
    out = []
    for sym, num, body, kernarg in kernels:
        out += [f"\t.globl\t{sym}", f"{sym}: ; @{sym}", "; %bb.0:"]
        out += [l.replace("LBB_", f"LBB{num}_") for l in body]
        out += ["\t.section\t.rodata", f"\t.amdhsa_kernel {sym}", "\t\t.amdhsa_group_segment_fixed_size 0",
                "\t\t.amdhsa_private_segment_fixed_size 0", f"\t\t.amdhsa_kernarg_size {kernarg}",
                "\t\t.amdhsa_next_free_vgpr 8", "\t\t.amdhsa_next_free_sgpr 16", "\t.end_amdhsa_kernel",
                f".Lfunc_end{num}:", f"\t.size\t{sym}, .Lfunc_end{num}-{sym}", "; Occupancy: 8"]
    return "\n".join(out) + "\n"


BODY = ["\ts_load_dwordx2 s[4:5], s[0:1], 0x10  ; a comment", "\ts_mov_b64 s[6:7], s[0:1]", "\ts_load_dword s8, s[6:7], 0x20",
        "\ts_waitcnt lgkmcnt(0)", "\tv_mov_b32_e32 v1, s8", "\tv_fma_f32 v2, v1, v1, v1", ".LBB_1:",
        "\tglobal_store_dword v0, v2, s[4:5]", "\ts_cbranch_scc1 .LBB_1", "\ts_endpgm"]


def run(tmp_path, capsys, old, new, *args):
    (tmp_path / "old.s").write_text(listing(old))
    (tmp_path / "new.s").write_text(listing(new))
    rc = kid.main([str(tmp_path / "old.s"), str(tmp_path / "new.s"), *args])
    return rc, capsys.readouterr().out


def verdict(out, name):
    return next(l for l in out.splitlines() if l.startswith(name))


def test_the_three_verdicts(tmp_path, capsys):
    moved = [l.replace("0x10", "0x18").replace("0x20", "0x28") for l in BODY]          # kernarg offsets only
    other_base = [l.replace("s8, s[6:7], 0x20", "s8, s[4:5], 0x28") for l in BODY]     # a load that is no kernarg load
    unfused = BODY[:5] + ["\tv_mul_f32_e32 v2, v1, v1", "\tv_add_f32_e32 v2, v2, v1"] + BODY[6:]
    old = [("same", 0, BODY, 64), ("shifted", 1, BODY, 64), ("rebased", 2, BODY, 64), ("unfused", 3, BODY, 64)]
    new = [("shifted", 0, moved, 72), ("same", 1, BODY, 64), ("rebased", 2, other_base, 64), ("unfused", 3, unfused, 64)]
    rc, out = run(tmp_path, capsys, old, new)
    assert rc == 0
    assert verdict(out, "same").endswith("identical")               # the function number in the labels does not count
    assert "kernarg-only (3 lines)" in verdict(out, "shifted")      # two loads and .amdhsa_kernarg_size
    assert verdict(out, "rebased").endswith("differs")
    assert verdict(out, "unfused").endswith("differs")
    detail = out[out.index("unfused -> unfused: differs"):]
    assert "VGPR 8 / 8  SGPR 16 / 16  scratch 0 / 0  LDS 0 / 0" in detail
    assert "DIFFERENT: v_add_f32_e32, v_fma_f32, v_mul_f32_e32" in detail
    assert "v_fma_f32 1 / 0" in detail and "v_mul_f32_e32 0 / 1" in detail


def test_map_pairs_a_renamed_kernel_and_a_missing_one_fails(tmp_path, capsys):
    old, new = [("tail_rng", 0, BODY, 64)], [("tail_T", 0, BODY, 64)]
    rc, out = run(tmp_path, capsys, old, new)
    assert rc == 1 and "no partner" in verdict(out, "tail_rng") and "new" in verdict(out, "-")
    rc, out = run(tmp_path, capsys, old, new, "--map", "tail_rng=tail_T")
    assert rc == 0 and verdict(out, "tail_rng").endswith("identical")
