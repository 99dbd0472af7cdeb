"""The launch plans of the GroupNorm(+Swish) forward and backward restated in pure Python -- gn_plan (csrc/norm.hip: the
eleven gn_fwd_kernel<NV, NT> instantiations by n4 = cpg HW / 4, the general kernels of csrc/norm_any.hip, the ten
gn_bwd_fused_kernel<NV, NT, SEG> instantiations, the two-kernel backward with its chunks and add_inplace launches, and
every refusal) -- with the plan-class enumeration behind tests/test_gpu_gn_plan.py and the inputs, float64 / stock fp32
references, the CPU fp32 model of the kernels and its seven wrong variants that those tests share.

The coverage keys of a case are class_keys(case): one key per independent decision (forward instantiation x edge, channel
shift, Swish, plain / concatenated input; the general kernel by the way it is reached and by group size; where the
concatenation boundary falls; backward instantiation x edge x map; the two-kernel path's map, chunks, rows per workgroup
and add_inplace tail; refusals).  required_keys() derives the keys that must be covered from the tables alone; cases()
holds one representative per key, built directly at the cheapest point of the domain that has the key: HW = 4 (a 2 x 2
map, n4 = cpg) wherever the key does not name a map, S = 2 views and 2 groups unless the key asks otherwise (a view /
group index mix-up then cannot pass), gamma and beta different per channel (cond_ref.gn_params).

Domain: S in {1, 2, 3}, groups in {1, 2, 3, 32}, at most MAX_FLOATS = 2^21 floats per tensor; the most expensive class
(the general forward reached from a 2 x 2 map, n4 = 32769) has one 131076-float group at S = 2, groups = 2: a quarter of
the limit, so over_cap_classes() is empty.  Groups of one or two elements are NOT in the domain: their variance is 0 or
nearly so, and stock fp32 CPU torch itself errs by more than cond_ref.CAP on dx there (measured: 5e-3 at n = 2, a
non-finite scale at n = 1).  From n = 3 on the stock fp32 error stays at or below 1.5e-5 (probed: n = 3 .. 259 on small maps,
n = 6913 on one long row, n = 131072 .. 131074 with and without Swish).

The arithmetic works on Python ints and numpy arrays alike: tests/test_gn_plan_host.py pins it to libvf_hip.so (vf_gn_plan,
vf_gn_bwd_emits_rowsum) on the whole domain at once.  Imports no GPU code."""
import collections
import functools

import numpy as np
import torch

import cond_ref as cr

MAX_FLOATS = 1 << 21
GROUPS_DOMAIN = (1, 2, 3, 32)
RATIO, SIGMA = 10, 1.0                                  # cond_ref.gn_input's group offset and spread
SEED = 61

# vf_gn_plan's out[12]
FIELDS = ("fwd", "fnv", "fnt", "bwd", "bnv", "bnt", "seg", "lds", "chunks", "adds", "rowsum", "cpg")
REJECTED, FWD_REG, FWD_ANY = 0, 1, 2
BWD_FUSED16, BWD_FUSED64, BWD_TWO, BWD_ANY = 1, 2, 3, 4
FWD_NAMES = ("rejected", "gn_fwd_kernel", "gn_any_fwd_kernel")
BWD_NAMES = ("rejected", "gn_bwd_fused_kernel<.,256,16>", "gn_bwd_fused_kernel<.,.,64>", "gn_bwd_rows+dx", "gn_any_bwd_kernel")
FWD_TABLE = ((64, 1, 64), (256, 1, 256), (512, 2, 256), (1024, 4, 256), (2048, 8, 256), (3072, 12, 256), (4096, 16, 256),
             (6144, 12, 512), (8192, 16, 512), (16384, 16, 1024), (32768, 32, 1024))       # (largest n4, NV, NT)
BWD16_TABLE = ((256, 1, 256), (512, 2, 256), (1024, 4, 256))                                # HW = 64
BWD64_TABLE = ((256, 1, 256), (512, 2, 256), (1024, 4, 256), (2048, 8, 256), (4096, 8, 512), (6144, 12, 512), (8192, 8, 1024))
SHIFT_HW = (4, 8, 16, 32, 64, 128, 256, 1024, 4096)
MAPS = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (2, 2), 8: (2, 4), 12: (3, 4), 15: (3, 5), 16: (4, 4), 25: (5, 5), 32: (4, 8),
        60: (6, 10), 64: (8, 8), 128: (8, 16), 256: (16, 16), 1024: (32, 32), 4096: (64, 64)}


# ------------------------------------------------------------------------------------------------ the planner
def _table(n4, table):
    nv, nt = np.zeros_like(n4), np.zeros_like(n4)
    for lim, v, t in reversed(table):
        nv, nt = np.where(n4 <= lim, v, nv), np.where(n4 <= lim, t, nt)
    return nv, nt


def plan_arrays(C, HW, groups, cat=0, C1=0, has_addend=0, has_addend2=0, has_dx2=0):
    """gn_plan (csrc/norm.hip) -> dict of FIELDS; every argument an int or an int64 array (broadcast together)."""
    C, HW, groups, cat, C1, a1, a2, dx2 = np.broadcast_arrays(*(np.asarray(v, dtype=np.int64) for v in
                                                                (C, HW, groups, cat, C1, has_addend, has_addend2, has_dx2)))
    cat, a1, a2, dx2 = cat != 0, a1 != 0, a2 != 0, dx2 != 0
    valid = (groups > 0) & (C % np.where(groups > 0, groups, 1) == 0)
    cpg = np.where(valid, C // np.where(groups > 0, groups, 1), 0)
    pow2 = (HW >= 4) & ((HW & (HW - 1)) == 0)
    n4 = cpg * HW // 4
    cat_ok = ~cat | ((C1 > 0) & (C1 < C))
    gen = ~pow2 | (n4 > 32768)
    fnv, fnt = _table(n4, FWD_TABLE)
    fwd = np.where(gen, np.where(cat | (HW < 1), REJECTED, FWD_ANY), np.where(cat_ok, FWD_REG, REJECTED))
    fwd = np.where(valid, fwd, REJECTED)
    reg = fwd == FWD_REG
    f16, f64 = pow2 & (HW == 64) & (n4 <= 1024), pow2 & (HW >= 256) & (n4 <= 8192)
    cat_bad = cat & (~cat_ok | ~dx2 | (a1 & ~a2) | ~(f16 | f64))
    bwd = np.where(~pow2, np.where(cat | (HW < 1), REJECTED, BWD_ANY),
                   np.where(cat_bad, REJECTED, np.where(f16, BWD_FUSED16, np.where(f64, BWD_FUSED64, BWD_TWO))))
    bwd = np.where(valid, bwd, REJECTED)
    v16, t16 = _table(n4, BWD16_TABLE)
    v64, t64 = _table(n4, BWD64_TABLE)
    fused = (bwd == BWD_FUSED16) | (bwd == BWD_FUSED64)
    bnv = np.where(bwd == BWD_FUSED16, v16, np.where(bwd == BWD_FUSED64, v64, 0))
    bnt = np.where(bwd == BWD_FUSED16, t16, np.where(bwd == BWD_FUSED64, t64, 0))
    two = bwd == BWD_TWO
    z = np.zeros_like(n4)
    return dict(fwd=fwd, fnv=np.where(reg, fnv, 0), fnt=np.where(reg, fnt, 0), bwd=bwd, bnv=bnv, bnt=bnt,
                seg=np.where(bwd == BWD_FUSED16, 16, np.where(bwd == BWD_FUSED64, 64, 0)),
                lds=np.where(fused, (bnt // 64) * cpg * 12, 0), chunks=np.where(two, np.maximum((n4 + 1023) // 1024, 1), 0),
                adds=np.where(two, a1.astype(np.int64) + a2, 0), rowsum=fused.astype(np.int64) + z, cpg=cpg + z, n4=n4 + z)


def emits_rowsum(C, HW, groups):
    """vf_gn_bwd_emits_rowsum: a read of the plain plan."""
    return plan_arrays(C, HW, groups, 0, C)["rowsum"]


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "S C H W groups C1 silu why")
ADDEND_STATES = ("none", "addend", "both")


def mk(S, cpg, HW, groups=2, C1=0, silu=1, why=""):
    H, W = MAPS[HW]
    return Case(int(S), int(cpg * groups), H, W, int(groups), int(C1), int(silu), why)


def case_id(c):
    return f"S{c.S}-C{c.C}g{c.groups}-{c.H}x{c.W}" + (f"-cat{c.C1}" if c.C1 else "") + ("-silu" if c.silu else "")


def floats(c):
    return c.S * c.C * c.H * c.W


def plan(c, state="none", cat=None):
    """The plan of case c as plain ints; state: one of ADDEND_STATES (a concatenated input takes "none" or "both", its two
    addends being the two parts of one tensor); cat: None = as the case says."""
    cat = bool(c.C1) if cat is None else cat
    a1, a2 = state != "none", state == "both"
    d = plan_arrays(c.C, c.H * c.W, c.groups, int(cat), c.C1 if cat else c.C, int(a1), int(a2), int(cat))
    return {k: int(v) for k, v in d.items()}


def fields(d):
    return [d[k] for k in FIELDS]


def _bounds(table, n4):
    """(smallest n4, largest n4) of the table row that n4 selects."""
    lo = 1
    for lim, _, _ in table:
        if n4 <= lim:
            return lo, lim
        lo = lim + 1
    raise ValueError(n4)


def cat_kinds(c):
    """Where the concatenation boundary C1 falls."""
    if not c.C1:
        return []
    cpg = c.C // c.groups
    k = ["on a group edge" if c.C1 % cpg == 0 else "inside a group"]
    if c.C1 % cpg and c.C1 < cpg:
        k.append("inside the first group")
    if c.C1 % cpg and c.C1 > c.C - cpg:
        k.append("inside the last group")
    if c.C1 % 4:
        k.append("C1 % 4 != 0")
    return k


def _any_origin(c):
    HW = c.H * c.W
    if HW < 4:
        return "HW < 4"
    if HW & (HW - 1):
        return "HW not a power of two"
    return f"power-of-two map {HW}"


def _any_size(n):
    return "n < 256" if n < 256 else "n % 256 == 0" if n % 256 == 0 else "n > 256, n % 256 != 0"


def class_keys(c):
    """The coverage keys of case c (forward, then the backward every addend state of which the GPU test runs)."""
    d = plan(c)
    HW, cpg, n4 = c.H * c.W, d["cpg"], d["n4"]
    kind = "cat" if c.C1 else "plain"
    keys = []
    if d["fwd"] == FWD_REG:
        nv, nt = d["fnv"], d["fnt"]
        lo, hi = _bounds(FWD_TABLE, n4)
        edges = [("threshold", n4 == hi), ("smallest", n4 == lo), ("partly filled slot", n4 % nt != 0),
                 ("empty slot", nv > 1 and n4 <= (nv - 1) * nt)]
        keys += [("fwd", nv, nt, e) for e, on in edges if on]
        keys += [("fwd shift", nv, nt, HW), ("fwd silu", nv, nt, c.silu), ("fwd input", nv, nt, kind)]
    elif d["fwd"] == FWD_ANY:
        keys.append(("fwd any", _any_origin(c), _any_size(cpg * HW)))
    keys += [("cat", k, FWD_NAMES[d["fwd"]], BWD_NAMES[d["bwd"]]) for k in cat_kinds(c)]
    if d["bwd"] in (BWD_FUSED16, BWD_FUSED64):
        lo, hi = _bounds(BWD16_TABLE if d["bwd"] == BWD_FUSED16 else BWD64_TABLE, n4)
        step = HW // 4                                   # n4 moves in steps of one channel
        edge = "threshold" if n4 + step > hi else "smallest" if n4 - step < lo else "inside"
        keys.append(("bwd", d["seg"], d["bnv"], d["bnt"], HW, edge))
        if edge == "threshold" and n4 - step < lo:
            keys.append(("bwd", d["seg"], d["bnv"], d["bnt"], HW, "smallest"))
        keys.append(("bwd input", d["seg"], d["bnv"], d["bnt"], kind))
    elif d["bwd"] == BWD_TWO:
        keys += [("bwd two", HW, "first past the fused limit" if (HW == 64 and cpg == 65) or (HW >= 256 and n4 - HW // 4 <= 8192) else ""),
                 ("bwd two chunks", "1" if d["chunks"] == 1 else "2" if d["chunks"] == 2 else "> 2"),
                 ("bwd two rows", c.S * c.C % 4), ("bwd two add tail", "ragged" if (floats(c) // 4) % 256 else "whole")]
    elif d["bwd"] == BWD_ANY:
        keys.append(("bwd any", _any_origin(c), _any_size(cpg * HW)))
    elif c.C1:
        keys.append(("reject", "cat where the fused backward does not apply"))
    return keys


def required_keys():
    """The keys the issue names, from the tables alone (reachability by arithmetic, not by looking at cases())."""
    req = set()
    lo = 1
    for hi, nv, nt in FWD_TABLE:
        req |= {("fwd", nv, nt, "threshold"), ("fwd", nv, nt, "smallest"), ("fwd", nv, nt, "partly filled slot")}
        if nv > 1 and lo <= (nv - 1) * nt:               # (2, 256): n4 >= 257 always reaches slot 1
            req.add(("fwd", nv, nt, "empty slot"))
        for HW in SHIFT_HW:
            if (hi * 4 // HW) * HW // 4 >= lo:
                req.add(("fwd shift", nv, nt, HW))
        req |= {("fwd silu", nv, nt, 0), ("fwd silu", nv, nt, 1), ("fwd input", nv, nt, "plain"), ("fwd input", nv, nt, "cat")}
        lo = hi + 1
    req |= {("fwd any", "power-of-two map 4", _any_size(4 * 32769)), ("fwd any", "power-of-two map 4096", _any_size(33 * 4096))}
    for origin in ("HW not a power of two", "HW < 4"):
        req |= {("fwd any", origin, "n < 256"), ("fwd any", origin, "n > 256, n % 256 != 0"),
                ("bwd any", origin, "n < 256"), ("bwd any", origin, "n > 256, n % 256 != 0")}
    for fwd, bwd in ((FWD_REG, REJECTED), (FWD_REG, BWD_FUSED16), (FWD_REG, BWD_FUSED64)):
        for k in ("on a group edge", "inside a group", "inside the first group", "inside the last group", "C1 % 4 != 0"):
            req.add(("cat", k, FWD_NAMES[fwd], BWD_NAMES[bwd]))
    for table, seg, maps in ((BWD16_TABLE, 16, (64,)), (BWD64_TABLE, 64, (256, 1024, 4096))):
        lo = 1
        for hi, nv, nt in table:
            for HW in maps:
                if (hi * 4 // HW) * HW // 4 >= lo:
                    req |= {("bwd", seg, nv, nt, HW, "threshold"), ("bwd", seg, nv, nt, HW, "smallest")}
            req |= {("bwd input", seg, nv, nt, "plain"), ("bwd input", seg, nv, nt, "cat")}
            lo = hi + 1
    req |= {("bwd two", HW, "") for HW in (4, 8, 16, 32, 128)}
    req |= {("bwd two", 64, "first past the fused limit"), ("bwd two", 256, "first past the fused limit")}
    req |= {("bwd two chunks", k) for k in ("1", "2", "> 2")} | {("bwd two rows", r) for r in range(4)}
    req |= {("bwd two add tail", "ragged"), ("reject", "cat where the fused backward does not apply")}
    return req


def _build():
    out = []
    add = lambda *a, **k: out.append(mk(*a, **k))
    # forward: every instantiation on its edges, on a 2 x 2 map (n4 = cpg)
    lo = 1
    for i, (hi, nv, nt) in enumerate(FWD_TABLE):
        add(2, hi, 4, silu=1, why=f"fwd ({nv}, {nt}) on its threshold n4 = {hi}")
        add(2, lo, 4, silu=0, why=f"fwd ({nv}, {nt}) at its smallest n4 = {lo}")
        add(2, hi - 1, 4, silu=1, why=f"fwd ({nv}, {nt}) with the last slot partly filled")
        if nv > 1 and lo <= (nv - 1) * nt:
            n4 = max(lo + 1, (nv - 2) * nt + nt // 2 + 1)
            assert n4 <= (nv - 1) * nt
            add(2, n4, 4, silu=0, why=f"fwd ({nv}, {nt}) with slot {nv - 1} wholly out of range (n4 = {n4})")
        for j, HW in enumerate(SHIFT_HW[1:]):            # the channel shift: the largest group of this map that selects it
            cpg = hi * 4 // HW
            if cpg * HW // 4 >= lo:
                add(2, cpg, HW, silu=(i + j) % 2, why=f"fwd ({nv}, {nt}) at HW = {HW}")
        # a concatenated input per instantiation: the boundary kinds in turn
        C1 = (hi, hi + hi // 2 + 1, 1, 2 * hi - 1)[i % 4]
        add(2, hi, 4, C1=C1, silu=i % 2, why=f"fwd ({nv}, {nt}) on a concatenation split at {C1}")
        lo = hi + 1
    # the general forward / backward
    add(2, 32769, 4, silu=1, why="n4 = 32769 on a 2 x 2 map: general forward, two-kernel backward with 33 chunks")
    add(2, 33, 4096, silu=0, why="the first over-size group of a 64 x 64 map (n4 = 33792): general forward")
    for HW, cpg, g, S, silu in ((15, 3, 2, 2, 1), (15, 20, 2, 2, 0), (12, 64, 2, 2, 1), (25, 11, 3, 3, 1), (60, 2, 32, 2, 0),
                                (1, 5, 2, 2, 1), (1, 300, 2, 2, 0), (2, 3, 3, 2, 0), (3, 3, 2, 3, 1), (3, 100, 2, 2, 1)):
        add(S, cpg, HW, groups=g, silu=silu, why=f"general kernels: HW = {HW}, a group of {cpg * HW}")
    # where the concatenation boundary falls: forward only (2 x 2), 16-lane fused backward (8 x 8), 64-lane (16 x 16)
    for HW, cpg in ((4, 6), (64, 4), (256, 4)):
        C = 3 * cpg
        for C1 in (cpg, cpg + cpg // 2, 1, C - 1):
            add(2, cpg, HW, groups=3, C1=C1, silu=C1 % 2, why=f"concatenation split at {C1} of {C}, groups of {cpg}, HW = {HW}")
    # backward: the 16-lane fused kernels either side of 256, 512 and 1024, and the first group past them
    for cpg in (1, 16, 17, 32, 33, 64, 65):
        add(2, cpg, 64, silu=cpg % 2, why=f"8 x 8 backward at n4g = {16 * cpg}")
    for i, (hi, nv, nt) in enumerate(BWD16_TABLE):
        add(2, hi // 16, 64, C1=(hi // 16 + 1, hi // 16, 2 * (hi // 16) - 1)[i], silu=i % 2, why=f"8 x 8 fused backward ({nv}, 256, 16) on a concatenation")
    # the 64-lane fused kernels at every map that reaches them, threshold and smallest, and on a concatenation
    lo = 1
    for i, (hi, nv, nt) in enumerate(BWD64_TABLE):
        for HW in (256, 1024, 4096):
            c_hi, c_lo = hi * 4 // HW, -(-lo * 4 // HW)
            for cpg in dict.fromkeys((c_hi, c_lo)):
                if c_lo <= c_hi:
                    add(2, cpg, HW, silu=(i + cpg) % 2, why=f"fused backward ({nv}, {nt}, 64) at HW = {HW}, n4g = {cpg * HW // 4}")
        cpg = hi // 64
        add(2, cpg, 256, C1=(cpg, cpg + 1, 1, 2 * cpg - 1)[i % 4], silu=i % 2, why=f"fused backward ({nv}, {nt}, 64) on a concatenation")
        lo = hi + 1
    add(2, 129, 256, silu=1, why="16 x 16 with n4g = 8256: the first group past the fused limit")
    # the two-kernel path: its maps, rows per workgroup (S C % 4 = 0 .. 3), chunks
    for HW in (4, 8, 16, 32, 128):
        add(2, 3, HW, silu=HW % 3 % 2, why=f"two-kernel backward at HW = {HW}")
    for S, g, cpg in ((3, 3, 1), (3, 2, 3), (3, 3, 3)):
        add(S, cpg, 16, groups=g, silu=S * g * cpg % 2, why=f"two-kernel backward with S C % 4 = {S * g * cpg % 4}")
    add(2, 8, 32, groups=32, silu=1, why="32 groups on the two-kernel path, add_inplace over whole workgroups")
    add(2, 2, 64, groups=32, silu=0, why="32 groups on an 8 x 8 map")
    add(1, 40, 16, groups=1, silu=1, why="one view, one group")
    return out


@functools.lru_cache(maxsize=None)
def _enumerate():
    found = collections.OrderedDict()
    for c in _build():
        found.setdefault(c[:-1], []).append(c.why)
    return tuple(Case(*k, "; ".join(dict.fromkeys(v))) for k, v in found.items())


def cases():
    return list(_enumerate())


def case_classes():
    return {k for c in cases() for k in class_keys(c)}


def over_cap_classes():
    """Required keys whose cheapest representative needs more than MAX_FLOATS floats per tensor.  None: the largest group
    any key asks for is n4 = 33792 (135168 floats), at S = 2 and two groups 540672 floats = 0.26 MAX_FLOATS."""
    return {k: "no case under the float limit" for k in required_keys() - case_classes()}


def hygiene_cases():
    """The cheapest case per (forward route and instantiation, backward route and instantiation, plain / cat)."""
    pick = {}
    for c in sorted(cases(), key=lambda c: (floats(c), case_id(c))):
        d = plan(c)
        pick.setdefault((d["fwd"], d["fnv"], d["fnt"], d["bwd"], d["bnv"], d["bnt"], bool(c.C1)), c)
    return list(pick.values())


# rejected calls: (C, HW, groups, cat, C1, has_addend, has_addend2, has_dx2) -> which direction refuses, why
REJECTIONS = (
    ((12, 64, 0, 0, 12, 0, 0, 0), "both", "groups <= 0"),
    ((12, 64, -2, 0, 12, 0, 0, 0), "both", "groups <= 0"),
    ((12, 64, 5, 0, 12, 0, 0, 0), "both", "C % groups != 0"),
    ((12, 60, 3, 1, 4, 0, 0, 1), "both", "cat with HW not a power of two"),
    ((12, 2, 3, 1, 4, 0, 0, 1), "both", "cat with HW < 4"),
    ((12, 16, 3, 1, 4, 0, 0, 1), "bwd", "cat where the fused backward does not apply"),
    ((2 * 65, 64, 2, 1, 4, 0, 0, 1), "bwd", "cat where the fused backward does not apply"),
    ((12, 64, 3, 1, 0, 0, 0, 1), "both", "C1 <= 0"),
    ((12, 64, 3, 1, -3, 0, 0, 1), "both", "C1 <= 0"),
    ((12, 64, 3, 1, 12, 0, 0, 1), "both", "C1 >= C"),
    ((12, 256, 3, 1, 13, 0, 0, 1), "both", "C1 >= C"),
    ((12, 64, 3, 1, 4, 1, 0, 1), "bwd", "cat with addend but no addend2"),
    ((12, 256, 3, 1, 4, 0, 0, 0), "bwd", "cat without dx2"),
)


# ------------------------------------------------------------------------------------------------ the models' layers
def model_layers():
    """(C, H, groups, C1 | 0) of every GroupNorm of the SMALL and TINY networks (view_fusion_amd/unet.py): the two of each
    residual block (the first one of a decoder block over [x | skip], C1 = the channels of x), each attention block's,
    the final one."""
    from conftest import SMALL, TINY
    from view_fusion_amd import UNet
    out = set()
    for hp in (SMALL, TINY):
        net = UNet(**hp)
        g = hp["norm_groups"]

        def block(layer, H, C1):
            rb = layer.res_block
            n1, n2 = rb.block1["block"]["0"], rb.block2["block"]["0"]
            out.add((n1.num_channels, H, g, C1 if C1 else 0))
            if C1:
                out.add((n1.num_channels, H, g, 0))      # (materialised where ops.cat_fusable says no)
            out.add((n2.num_channels, H, g, 0))
            if getattr(layer, "attn", None) is not None:
                out.add((layer.attn.norm.num_channels, H, g, 0))
            return rb.block2["block"]["3"].out_channels

        def level(conv):
            return hp["image_size"] >> conv._vf_geom[0]
        ch = None
        for layer in list(net.downs) + list(net.mid):
            if hasattr(layer, "res_block"):
                ch = block(layer, level(layer.res_block.block1["block"]["3"]), 0)
        for layer in net.ups:
            if hasattr(layer, "res_block"):
                ch = block(layer, level(layer.res_block.block1["block"]["3"]), ch)
        fc = net.final_conv["block"]
        out.add((fc["0"].num_channels, hp["image_size"], g, 0))
    return sorted(out)


def plan_class(C, HW, groups, C1):
    """What separates two launches for the kernels: routes, instantiations, the map's channel shift, where a boundary falls."""
    c = Case(2, C, 1, HW, groups, C1, 1, "")
    keys = class_keys(c)
    return [k for k in keys if k[0] in ("fwd shift", "fwd input", "fwd any", "cat", "bwd input", "bwd any", "reject")] \
        + [k[:2] for k in keys if k[0] == "bwd two"] + [k[:5] for k in keys if k[0] == "bwd"]


# ------------------------------------------------------------------------------------------------ inputs and references
def inputs(c):
    """-> dict(x, gamma, beta, dy, a1, a2), float32 on the CPU, seeded; a1 / a2: the addends, drawn like x."""
    x = cr.gn_input(c.S, c.C, c.H, c.W, RATIO, SIGMA, SEED, groups=c.groups)
    gamma, beta, dy = cr.gn_params(c.S, c.C, c.H, c.W, SEED)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, a1=cr.gn_input(c.S, c.C, c.H, c.W, RATIO, SIGMA, SEED + 10, groups=c.groups),
                a2=cr.gn_input(c.S, c.C, c.H, c.W, RATIO, SIGMA, SEED + 20, groups=c.groups))


OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
TOLS = dict(y=cr.TOL["gn_fwd"], mean=cr.TOL["gn_fwd"], rstd=cr.TOL["gn_fwd"], dx=cr.TOL["gn_bwd"], dgamma=cr.TOL["gn_bwd"],
            dbeta=cr.TOL["gn_bwd"])


def _stats(x, groups, dt):
    xg = x.to(dt).reshape(x.shape[0], groups, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + cr.EPS)


def refs(c, t, silu):
    """-> (r64, r32): dicts of OUTPUTS (dx without addends) and, in r64, "rowsum" = the float64 row sums of dx; r64 from
    cond_ref's float64 restatement, r32 from stock fp32 torch on the CPU (F.group_norm, torch.native_group_norm's statistics)."""
    a, b = cr.gn_ref(t["x"], t["gamma"], t["beta"], t["dy"], bool(silu), c.groups)
    r64, r32 = dict(zip(("y", "dx", "dgamma", "dbeta"), a)), dict(zip(("y", "dx", "dgamma", "dbeta"), b))
    m, r = _stats(t["x"], c.groups, torch.float64)
    r64.update(mean=m, rstd=r, rowsum=r64["dx"].sum((2, 3)), rowabs=float(r64["dx"].abs().sum((2, 3)).max()))
    _, m32, r32_ = torch.native_group_norm(t["x"], t["gamma"], t["beta"], c.S, c.C, c.H * c.W, c.groups, cr.EPS)
    r32.update(mean=m32.reshape(c.S, c.groups), rstd=r32_.reshape(c.S, c.groups))
    return r64, r32


def with_addends(r, t, state, dt):
    """dx of a reference with the addends of `state` (the arithmetic of the references stays in their own precision)."""
    dx = r["dx"]
    if state != "none":
        dx = dx + t["a1"].to(dt)
    if state == "both":
        dx = dx + t["a2"].to(dt)
    return dict(r, dx=dx)


def cat_addend(t, c):
    """A concatenated input's two addends are the two parts of ONE tensor: the state "both" adds a1 only."""
    return dict(t, a2=torch.zeros_like(t["a2"]))


def judge_all(got, r64, r32, names=OUTPUTS):
    """-> [(name, err, e, bound, ok)] under cond_ref.judge with the unchanged family tolerances."""
    return [(n, *cr.judge(got[n], r64[n], r32[n], TOLS[n])) for n in names if got.get(n) is not None]


# ------------------------------------------------------------------------------------------------ the CPU fp32 model
MUTANTS = ("clamped_stats", "neighbour_affine", "var_n_minus_1", "drop_addend2", "no_s2_term", "cat_boundary_off", "swap_view_group")


def mutant_applies(c, d, m, state):
    """clamped_stats     the register forward with lanes clamped onto the group's last float4 (n4 < NV NT)
    neighbour_affine  any case with two channels or more
    var_n_minus_1     groups of at most 32768 elements: rstd moves by 1 / (2 n) >= 1.5e-5, above gn_fwd's 1e-5
    drop_addend2      the addend state "both"
    no_s2_term        every case
    cat_boundary_off  a concatenated input
    swap_view_group   two views and two groups or more"""
    if m == "clamped_stats":
        return d["fwd"] == FWD_REG and d["n4"] < d["fnv"] * d["fnt"]
    if m == "neighbour_affine":
        return c.C >= 2
    if m == "var_n_minus_1":
        return d["cpg"] * c.H * c.W <= 32768
    if m == "drop_addend2":
        return state == "both"
    if m == "no_s2_term":
        return True
    if m == "cat_boundary_off":
        return bool(c.C1)
    if m == "swap_view_group":
        return c.S >= 2 and c.groups >= 2
    raise KeyError(m)


def kernel_model(c, t, silu, state="none", mutate=None):
    """The kernels' arithmetic in float32 on the CPU (two-pass statistics over the group, y = x (gamma rstd) + (beta - mean
    gamma rstd), dx = rstd (dz gamma - (s1 + xhat s2)) + addends) -> dict of OUTPUTS.  mutate, one of MUTANTS:
      clamped_stats     the lanes clamped onto the group's last float4 are counted in the sums of the statistics
      neighbour_affine  a channel's last float4 takes gamma / beta of the next channel
      var_n_minus_1     the variance divides by n - 1
      drop_addend2      addend2 is not added (a concatenated input: the second part of dx gets no addend)
      no_s2_term        dx without the s2 xhat term
      cat_boundary_off  the boundary one channel late: channel C1 is read behind the first tensor's last channel
      swap_view_group   mean / rstd stored at [group][view]"""
    d = plan(c)
    assert mutate is None or (mutate in MUTANTS and mutant_applies(c, d, mutate, state))
    S, C, G, HW = c.S, c.C, c.groups, c.H * c.W
    cpg, n = C // G, (C // G) * c.H * c.W
    x, gamma, beta, dy = t["x"].reshape(S, C, HW).clone(), t["gamma"], t["beta"], t["dy"].reshape(S, C, HW)
    if mutate == "cat_boundary_off":                     # x1 + (s C1 + C1) HW = channel 0 of the next view of x1
        x[:, c.C1] = x.roll(-1, 0)[:, 0]
    xg = x.reshape(S, G, n)
    extra = d["fnv"] * d["fnt"] - d["n4"] if mutate == "clamped_stats" else 0
    mean = (xg.sum(-1) + extra * xg[..., -4:].sum(-1)) / n
    dev = xg - mean[..., None]
    sq = (dev * dev).sum(-1) + extra * (dev[..., -4:] ** 2).sum(-1)
    rstd = 1.0 / torch.sqrt(sq / (n - 1 if mutate == "var_n_minus_1" else n) + cr.EPS)
    gam, bet = gamma[None, :, None].expand(S, C, HW).clone(), beta[None, :, None].expand(S, C, HW).clone()
    if mutate == "neighbour_affine":
        gam[:, :-1, -4:] = gamma[None, 1:, None]
        bet[:, :-1, -4:] = beta[None, 1:, None]
    mu_c, r_c = mean.repeat_interleave(cpg, 1)[..., None], rstd.repeat_interleave(cpg, 1)[..., None]
    ga = gam * r_c
    z = x * ga + (bet - mu_c * ga)
    y = z * torch.sigmoid(z) if silu else z
    mean_out, rstd_out = mean, rstd
    if mutate == "swap_view_group":
        mean_out, rstd_out = mean.t().reshape(S, G), rstd.t().reshape(S, G)
        mu_c, r_c = mean_out.repeat_interleave(cpg, 1)[..., None], rstd_out.repeat_interleave(cpg, 1)[..., None]
    xh = (x - mu_c) * r_c
    if silu:
        zz = xh * gam + bet
        sg = torch.sigmoid(zz)
        dz = dy * (sg * (1.0 + zz * (1.0 - sg)))
    else:
        dz = dy
    A, B = dz.sum(-1), (dz * xh).sum(-1)
    s1 = (gamma[None] * A).reshape(S, G, cpg).sum(-1).repeat_interleave(cpg, 1)[..., None] / n
    s2 = (gamma[None] * B).reshape(S, G, cpg).sum(-1).repeat_interleave(cpg, 1)[..., None] / n
    dx = r_c * (dz * gam - (s1 + (0 if mutate == "no_s2_term" else xh * s2)))
    if state != "none":
        dx = dx + t["a1"].reshape(S, C, HW)
    if state == "both":
        a2 = t["a2"].reshape(S, C, HW)
        if mutate == "drop_addend2":
            if c.C1:
                dx[:, c.C1:] = dx[:, c.C1:] - t["a1"].reshape(S, C, HW)[:, c.C1:]
        else:
            dx = dx + a2
    return dict(y=y.reshape(t["x"].shape), mean=mean_out, rstd=rstd_out, dx=dx.reshape(t["x"].shape), dgamma=B.sum(0), dbeta=A.sum(0))
