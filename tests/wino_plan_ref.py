"""The K-split tail plan of the two persistent Winograd kernels restated in pure Python (csrc/wino_plan.h and the host
functions of csrc/winograd24.hip -- "nested", F(2,3)xF(4,3) -- and csrc/winograd44f.hip -- "f44", F(4x4,3x3)), the
plan-class enumeration behind tests/test_gpu_wino_tail_plan.py, and the inputs / references its cases share.

A launch of T = tile groups x ceil(Cout/64) workgroup tiles over nch = ceil(Cin/8) chunks computes tiles [0, nfull) whole
on 256 persistent workgroups; each of the R = T - nfull tail tiles is cut into `split` K ranges [p per, min(nch, (p+1) per)),
per = ceil(nch/split), whose raw partial outputs a fix-up launch sums -- unless the workspace passed cannot hold them: then
every tile is computed whole (launch_plan).  The coverage key of a launch is its plan class (kernel, map width, split,
last range shorter than `per`).

tests/test_wino_plan_host.py pins every function here to libvf_hip.so's host functions over a grid and checks that every
class the SMALL / TINY layers reach is in cases().  Imports no GPU code."""
import collections
import functools
import math
import os

import torch
import torch.nn.functional as F

SLOTS = 256                 # one workgroup per CU (WINO_SLOTS)
TAIL_F = 2.5                # per-part overhead of a K-split tail part, in chunk-times (WINO_TAIL_F)
TAIL_G = 4.0                # cost of the fix-up launch, in chunk-times (WINO_TAIL_G)
CK, CO, TT = 8, 64, 32      # channels per chunk, output channels and output tiles per workgroup (both kernels)
KERNELS = ("nested", "f44")
MAPS = {"nested": (8, 16, 32, 64), "f44": (32, 64)}
PART_FLOATS = {"nested": CO * TT * 8, "f44": CO * TT * 16}      # raw partial output of one tail part (2x4 / 4x4 tiles)
ENTRY = {"nested": "vf_wino_conv_fwd", "f44": "vf_wino44_conv_fwd"}
TOL = {"nested": 2e-5, "f44": 3e-5}                             # y and dx (tests/test_gpu_kernels.py)
TOL_DW, TOL_DB, TOL_DRES = 1e-4, 2e-5, 1e-6
ENV = ("VF_WINO_TAIL_F", "VF_WINO_TAIL_G")

# the enumeration's domain: a superset of every stride-1 3x3 layer of the SMALL / TINY networks in both directions
# (channels up to 640) at S = 1 .. 23 B, B = 16
S_MAX, NCH_MAX, NCOT_MAX = 368, 80, 10
T_MAX = 5 * SLOTS           # beyond three rounds every plan is the unsplit one: larger T adds no class


def check_env(environ=None):
    """The library reads the tuning overrides once per process; a plan under them is not the plan restated here."""
    bad = [k for k in ENV if k in (os.environ if environ is None else environ)]
    if bad:
        raise RuntimeError(f"{', '.join(bad)} set: the Winograd tail-plan tests describe the default plan only; unset them")


check_env()


# ------------------------------------------------------------------------------------------------ csrc/wino_plan.h
def wino_tail_time(R, sp, nch, F):
    """Time of the tail in units of one whole tile: the parts run in ceil(R sp / 256) rounds of per + F chunk-times."""
    per = (nch + sp - 1) // sp
    fix = TAIL_G if (sp > 1 and F > 0.0) else 0.0
    return (float((R * sp + SLOTS - 1) // SLOTS) * (per + F) + fix) / (nch + F)


@functools.lru_cache(maxsize=None)
def wino_tail_plan(T, nch, F=TAIL_F):
    """-> (nfull, split)."""
    R = T % SLOTS
    if R == 0 or T // SLOTS >= 3:
        return T, 1
    best = 1
    for sp in range(2, min(8, nch // 4) + 1):
        per = (nch + sp - 1) // sp
        if (nch + per - 1) // per != sp:
            continue
        if wino_tail_time(R, sp, nch, F) < wino_tail_time(R, best, nch, F) - 1e-9:
            best = sp
    if best < 2:
        return T, 1
    return T - R, best


# ------------------------------------------------------------------------------------------------ the launchers' host side
def wino_groups(S, H, W):
    """Nested kernel: groups of 32 2x4 output tiles (256 pixels); an 8x8 map packs four views into one group."""
    tiles = (H // 2) * (W // 4)
    return S * (tiles // TT) if tiles >= TT else (S + TT // tiles - 1) // (TT // tiles)


def f44_groups(S, H, W):
    """F(4x4): groups of 32 4x4 output tiles (512 pixels)."""
    return S * ((H // 4) * (W // 4) // TT)


def groups(kernel, S, H, W):
    return wino_groups(S, H, W) if kernel == "nested" else f44_groups(S, H, W)


def supported(kernel, H, W, mode):
    """vf_wino_supported / vf_wino44_supported; mode 0 same, 2 up2 (H, W: the output size)."""
    return H == W and W in MAPS[kernel] and mode in (0, 2)


def _rup(v, m):
    return (v + m - 1) // m * m


def tiles_chunks(kernel, S, Cin, Cout, H, W):
    return groups(kernel, S, H, W) * (_rup(Cout, CO) // CO), _rup(Cin, CK) // CK


def ws_floats(kernel, S, Cin, Cout, H, W):
    """vf_wino_conv_ws_floats / vf_wino44_conv_ws_floats."""
    T, nch = tiles_chunks(kernel, S, Cin, Cout, H, W)
    nfull, split = wino_tail_plan(T, nch)
    return (T - nfull) * split * PART_FLOATS[kernel]


def fill_pct(kernel, S, Cin, Cout, H, W):
    """vf_wino_conv_fill_pct / vf_wino44_conv_fill_pct -> (percent, T): the tail priced without the per-part overhead."""
    T, nch = tiles_chunks(kernel, S, Cin, Cout, H, W)
    if T <= 0:
        return 0, T
    nfull, split = wino_tail_plan(T, nch, 0.0)
    time = (nfull + SLOTS - 1) // SLOTS + (wino_tail_time(T - nfull, split, nch, 0.0) if T > nfull else 0.0)
    return int(100.0 * T / SLOTS / time), T


def gn_fusable(S, Cin, Cout, H, W, mode, ngroups):
    """vf_wino_conv_gn_fusable: every tile a K-split tail tile, maps from 16x16, a (view, group) of at most 2048 2x4 tiles."""
    if not supported("nested", H, W, mode) or W < 16 or ngroups <= 0 or Cout % ngroups != 0:
        return False
    T, nch = tiles_chunks("nested", S, Cin, Cout, H, W)
    nfull, split = wino_tail_plan(T, nch)
    return nfull == 0 and 2 <= split <= 8 and (Cout // ngroups) * (H * W // 8) <= 2048


def describe(kernel, S, Cin, Cout, H, W):
    T, nch = tiles_chunks(kernel, S, Cin, Cout, H, W)
    nfull, split = wino_tail_plan(T, nch)
    per = (nch + split - 1) // split
    R = T - nfull
    return dict(T=T, nch=nch, nfull=nfull, R=R, split=split, per=per, last=nch - (split - 1) * per, parts=R * split)


KIND = {"nested": 1, "f44": 2}                                   # vf_wino_conv_plan's `kind` (ops.wino_kind's codes)
PLAN_FIELDS = ("T", "nch", "nfull", "split", "per", "npers", "conv_grid", "fixup_grid")      # ... and its out[8]
FIXUP_FLOATS = {"nested": 8, "f44": 4}                           # outputs one fix-up thread finishes (a 2x4 tile / a tile row)


def launch_plan(kernel, S, Cin, Cout, H, W, has_ws, ws):
    """vf_wino_conv_plan = csrc/wino_plan.h:wino_launch_plan, what the launchers execute: describe() after the clamp by the
    workspace actually passed (the parts do not fit, or no workspace: every tile whole), and the two grids."""
    d = describe(kernel, S, Cin, Cout, H, W)
    T, nch, nfull, split = d["T"], d["nch"], d["nfull"], d["split"]
    if not has_ws or d["parts"] * PART_FLOATS[kernel] > ws:
        nfull, split = T, 1
    nt, npers = T - nfull, min(nfull, SLOTS)
    return dict(T=T, nch=nch, nfull=nfull, split=split, per=(nch + split - 1) // split, npers=npers, conv_grid=npers + nt * split,
                fixup_grid=(nt * PART_FLOATS[kernel] // FIXUP_FLOATS[kernel] + 255) // 256)


# shader cycles per chunk of a workgroup tile, prologue + epilogue in chunk-times (ops/policy.py:_WINO_COST)
WINO_COST = {"nested": (3340.0, 4.2), "f44": (5390.0, 4.7)}


def cycles(kernel, S, Cin, Cout, H, W):
    """ops/policy.py:_wino_cycles, the model behind the choice between the two kernels: whole rounds of 256 tiles of
    (nch + F) chunk-times; a split tail runs ceil(parts / 256) rounds of (per + F), writes and re-reads its raw partials
    (2.5 passes at 2000 bytes per cycle) and pays 8000 cycles of fix-up launch."""
    ch, F = WINO_COST[kernel]
    d = describe(kernel, S, Cin, Cout, H, W)
    T, nch, parts = d["T"], d["nch"], d["parts"]
    if parts == 0:
        return -(-T // SLOTS) * (nch + F) * ch
    cyc = (T // SLOTS) * (nch + F) * ch + -(-parts // SLOTS) * (d["per"] + F) * ch
    return cyc + parts * PART_FLOATS[kernel] * 4 * 2.5 / 2000.0 + 8000.0


def plan_class(kernel, S, Cin, Cout, H, W):
    d = describe(kernel, S, Cin, Cout, H, W)
    return (kernel, W, d["split"], d["last"] < d["per"])


def ranges(nch, split):
    """The K ranges (in chunks) of a tail tile's parts, as the kernels cut them."""
    per = (nch + split - 1) // split
    return [(p * per, min(nch, (p + 1) * per)) for p in range(split)]


# ------------------------------------------------------------------------------------------------ the case list
Case = collections.namedtuple("Case", "kernel S Cin Cout H mode why")


def case_id(c):
    return f"{c.kernel}-{c.H}-{c.mode}-S{c.S}-{c.Cin}x{c.Cout}"


# per (kernel, map) one case of each; the predicate sees describe()'s dict
SPECIALS = [
    ("nfull=256+split", lambda d: d["nfull"] == 256 and d["split"] > 1),
    ("nfull=512+split", lambda d: d["nfull"] == 512 and d["split"] > 1),
    ("3+rounds ragged", lambda d: d["T"] // SLOTS >= 3 and d["T"] % SLOTS != 0 and d["split"] == 1 and d["nfull"] % 8 != 0),
    ("parts>256", lambda d: d["parts"] > SLOTS),
    ("R=1", lambda d: d["R"] == 1),
    ("R=255", lambda d: d["R"] == 255),
    # (255 tail tiles times any split need two rounds of parts, which never beats one whole round: R = 255 is not
    # producible with a split.  The launch it stands for -- a last round one tile short -- is kept, as the plan runs it.)
    ("T%256=255", lambda d: d["T"] % SLOTS == 255),
]
RAGGED_CINS = tuple(range(60, 8 * NCH_MAX, 8))       # Cin = 4 mod 8 from the first depth that can split (100, 108, 132, ...)


def _tile_table(kernel, W, s_ok=lambda S: True):
    """T -> the cheapest (S, ncot) giving it: two or more views wherever T allows it (a view stride or a per-view bias
    cannot go wrong on one), then the fewest S ncot (the cost of a case is S Cin Cout H W), then the smaller S."""
    best = {}
    for S in range(1, S_MAX + 1):
        if not s_ok(S):
            continue
        g = groups(kernel, S, W, W)
        for ncot in range(1, NCOT_MAX + 1):
            T = g * ncot
            if T > T_MAX:
                break
            key = (S < 2, S * ncot, S)
            if T not in best or key < best[T][0]:
                best[T] = (key, S, ncot)
    return best


def _candidates(kernel, W, cins=None, s_ok=lambda S: True):
    """[(cost key, S, Cin, Cout, describe)] over the domain, cheapest first.  The plan sees only (T, nch): Cin = 8 nch
    (or the ragged depths `cins`) and Cout = 64 ncot are enough."""
    out = []
    for T, (_, S, ncot) in _tile_table(kernel, W, s_ok).items():
        for Cin in (cins if cins is not None else range(CK, CK * NCH_MAX + 1, CK)):
            d = describe(kernel, S, Cin, CO * ncot, W, W)
            assert d["T"] == T
            out.append(((S < 2, S * Cin * ncot, S, Cin, ncot), S, Cin, CO * ncot, d))
    out.sort(key=lambda r: r[0])
    return out


def _search(cands, pred):
    """The cheapest (S, Cin, Cout) among the candidates whose plan satisfies pred(describe), or None."""
    return next((r[1:4] for r in cands if pred(r[4])), None)


@functools.lru_cache(maxsize=None)
def _enumerate():
    found = collections.OrderedDict()      # (kernel, S, Cin, Cout, H, mode) -> [why]
    table = []                             # (kernel, W, rule, case id | "not producible")

    def add(kernel, W, mode, rule, hit):
        if hit is None:
            table.append((kernel, W, rule, "not producible"))
            return
        S, Cin, Cout = hit
        found.setdefault((kernel, S, Cin, Cout, W, mode), []).append(rule)
        table.append((kernel, W, rule, case_id(Case(kernel, S, Cin, Cout, W, mode, ""))))

    for kernel in KERNELS:
        for W in MAPS[kernel]:
            cands = _candidates(kernel, W)
            # 1. every plan class of the domain, cheapest representative
            for split in range(1, 9):
                for short in ((False,) if split == 1 else (False, True)):
                    rule = f"class split {split}{' short' if short else ''}"
                    add(kernel, W, "same", rule, _search(cands, lambda d: d["split"] == split and (d["last"] < d["per"]) == short))
            # 2. the shapes of a launch around the rounds of 256
            for rule, pred in SPECIALS:
                add(kernel, W, "same", rule, _search(cands, pred))
            # 3. the upsampling load with a short last range
            add(kernel, W, "up2", "up2 split short", _search(cands, lambda d: d["split"] > 1 and d["last"] < d["per"]))
            # 4. a ragged last chunk (Cin % 8 != 0) under a split tail
            add(kernel, W, "same", "Cin%8 split", _search(_candidates(kernel, W, cins=RAGGED_CINS), lambda d: d["split"] > 1))
    # 5. nested 8x8: the fix-up's second batch of partial loads on a ragged last group of four views
    for r in (1, 2, 3):
        add("nested", 8, "same", f"S%4={r} split>=5",
            _search(_candidates("nested", 8, s_ok=lambda S: S > 4 and S % 4 == r), lambda d: d["split"] >= 5))
    return tuple(Case(*k, "; ".join(v)) for k, v in found.items()), tuple(table)


def cases():
    return list(_enumerate()[0])


def case_table():
    """(kernel, map, rule, case id | "not producible") for every rule of the enumeration."""
    return list(_enumerate()[1])


def covered_classes():
    return {plan_class(c.kernel, c.S, c.Cin, c.Cout, c.H, c.H) for c in cases()}


def hygiene_cases():
    """Per (kernel, map) the split case with a short last range, per kernel one unsplit case of three or more rounds."""
    cs = cases()
    out = [next(c for c in cs if c.kernel == k and c.H == W and c.mode == "same"
                and (lambda d: d["split"] > 1 and d["last"] < d["per"])(describe(k, c.S, c.Cin, c.Cout, W, W)))
           for k in KERNELS for W in MAPS[k]]
    out += [next(c for c in cs if c.kernel == k and describe(k, c.S, c.Cin, c.Cout, c.H, c.H)["T"] >= 3 * SLOTS) for k in KERNELS]
    return out


def gn_cases(s_max=12, ngroups=32):
    """(S, Cin, Cout, H): the cheapest representative of every (map, split, short last range) class the fix-up's
    GroupNorm admits up to s_max views."""
    best = {}
    for W in (16, 32, 64):
        for S in range(1, s_max + 1):
            for Cout in range(ngroups, CO * NCOT_MAX + 1, ngroups):
                for Cin in range(CK, CK * NCH_MAX + 1, CK):
                    if not gn_fusable(S, Cin, Cout, W, W, 0, ngroups):
                        continue
                    key = (S < 2, S * Cin * Cout, S, Cin, Cout)
                    cls = plan_class("nested", S, Cin, Cout, W, W)[1:]
                    if cls not in best or key < best[cls][0]:
                        best[cls] = (key, S, Cin, Cout, W)
    return [best[k][1:] for k in sorted(best)]


# ------------------------------------------------------------------------------------------------ inputs and references
def rnd(*shape, seed=0, scale=1.0):
    """The inputs of tests/test_gpu_kernels.py: seeded uniform values in (-scale, scale)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def inputs(c):
    """-> dict(w, b, x, vb, res, gy): test_conv_fwd_bwd's tensors for case c (float32, CPU)."""
    Hin = c.H // 2 if c.mode == "up2" else c.H
    return dict(w=rnd(c.Cout, c.Cin, 3, 3, seed=5) / math.sqrt(c.Cin * 9), b=rnd(c.Cout, seed=6) * 0.1,
                x=rnd(c.S, c.Cin, Hin, Hin, seed=7), vb=rnd(c.S, c.Cout, seed=8) * 0.3,
                res=rnd(c.S, c.Cout, c.H, c.H, seed=9), gy=rnd(c.S, c.Cout, c.H, c.H, seed=10))


NAMES = ("y", "dx", "dW", "db", "dvb", "dres")


def tols(kernel):
    return (TOL[kernel], TOL[kernel], TOL_DW, TOL_DB, TOL_DB, TOL_DRES)


def conv_ref(t, mode, dtype, backward=True):
    """F.conv2d (+ bias + per-view bias + residual) in `dtype` on the CPU -> [y, dx, dW, db, dvb, dres] (or [y])."""
    lv = {k: t[k].to(dtype).clone().requires_grad_(backward) for k in ("x", "w", "b", "vb", "res")}
    inp = F.interpolate(lv["x"], scale_factor=2, mode="nearest") if mode == "up2" else lv["x"]
    y = F.conv2d(inp, lv["w"], lv["b"], padding=1) + lv["vb"][:, :, None, None] + lv["res"]
    if not backward:
        return [y.detach()]
    y.backward(t["gy"].to(dtype))
    return [y.detach()] + [lv[k].grad for k in ("x", "w", "b", "vb", "res")]


def conv_ksplit(t, chunk_ranges):
    """The forward as the tail does it, in fp32 on the CPU: one partial conv per K range (in 8-channel chunks), summed in
    order, then the epilogue.  With ranges(nch, split) this is the conv; the host test feeds it wrong ranges."""
    Cin = t["x"].shape[1]
    y = None
    for c0, c1 in chunk_ranges:
        lo, hi = min(CK * c0, Cin), min(CK * c1, Cin)
        p = F.conv2d(t["x"][:, lo:hi], t["w"][:, lo:hi], None, padding=1)
        y = p if y is None else y + p
    return y + t["b"][None, :, None, None] + t["vb"][:, :, None, None] + t["res"]
