"""The launch plans of the direct (non-Winograd) forward / dgrad convolutions restated in pure Python -- conv_fwd_plan
(csrc/conv.hip: conv_mfma_kernel, its tile size, SAFE instantiation, split-K factor, workspace clamp and the launch that
follows: plain reduce, reduce + GroupNorm variant, GroupNorm launch), the conv1x1_kernel<1|2> route (csrc/conv1x1.hip:
vfi_conv1x1_supported / vfi_conv1x1_halves at their natural policy) and the general kernel's fwd_plan (csrc/conv_any.hip)
-- with vf_conv_fwd_ws_floats, the plan-class enumeration behind tests/test_gpu_conv_plan.py, and the inputs / references
/ CPU split model its cases share.

A launch covers the output with nblk workgroup tiles of 64 npt pixels x 64 channels and cuts K (the nch chunks of 8
channels x 9 taps, or of 32 channels for 1x1) into ks ranges [split nch / ks, (split + 1) nch / ks) (floor: uneven when
nch % ks != 0); with ks > 1 every range writes one slab of partial sums into the workspace and a second launch adds the
slabs in index order, in batches, with bias / per-view bias / residual -- and the GroupNorm of vf_conv_fwd_gn where one
(view, group) fits a workgroup's registers.  vf_conv_fwd_ws_floats prices the split with 128-pixel tiles and no mode; the
launcher derives ks from the tile it takes, so "priced, fewer taken" and "priced, one taken" are plans of their own.

The coverage keys of a launch are class_keys(case): one key per independent decision (tile, split, channel padding, SAFE,
concatenation, split output, reduce, 1x1 threshold edge, general-kernel plan); cases() holds the cheapest representative
of every key over the domain below, and the hand-written SPECIALS.

The arithmetic works on Python ints and numpy arrays alike: the enumeration evaluates the very functions that
tests/test_conv_plan_host.py pins to libvf_hip.so (vf_conv_fwd_plan, vf_conv_fwd_ws_floats), on the whole domain at once.
Imports no GPU code."""
import collections
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import wgrad_plan_ref as wp

TOL = 2e-5                           # the project's tolerance for a conv output (tests/test_gpu_kernels.py; cond_ref.TOL["conv_gn"])
CAP_MACS = wp.CAP_MACS               # reference cost a case may have: S H W Cin Cout KS^2
ENV = ("VF_CONV_KSPLIT_WGS", "VF_CONV_NPT", "VF_CONV1X1_FORCE", "VF_CONV1X1_OLD", "VF_CONV1X1_NCW", "VF_CONV1X1_64")
KSPLIT_WGS = 256                     # choose_ksplit's budget: one workgroup per CU in a single round
CONV_MIN_WGS = 3 * 256               # 128-pixel tiles only where they fill the chip three times over
GROUPS = 32                          # the UNet's GroupNorm everywhere

# the enumeration's domain
S_MAX = wp.S_MAX
CHANNELS = wp.CHANNELS
# conv_fwd_impl's VF_CASE table: (KS, mode) -> output maps (mode 4: the dY map)
SPEC_MAPS = {(3, 0): (8, 16, 32, 64, 128), (3, 1): (8, 16, 32, 64), (3, 2): (16, 32, 64, 128), (3, 4): (8, 16, 32, 64),
             (1, 0): (8, 16, 32, 64, 128)}
# (H, W, KS, mode) of the general kernel: wgrad_plan_ref's shapes, the 1x1 conv on 6 x 10, the sub-pixel dgrad on 6 x 10
# and the two square power-of-two maps whose mode the specialised kernels lack (4 -> 8 Upsample, stride 2 onto 128 x 128)
ANY_SHAPES = wp.ANY_SHAPES + ((128, 128, 3, 1), (6, 10, 1, 0), (6, 10, 3, 4))
ROUTES = ("conv_mfma", "conv1x1<1>", "conv1x1<2>", "conv_any")
MFMA, ONE64, ONE128, ANY = 0, 1, 2, 3
RED_NONE, RED_PLAIN, RED_GN, RED_GN_LAUNCH, RED_PLAIN_GN_LAUNCH = 0, 1, 2, 3, 4
RED_NAMES = ("none", "plain", "reduce+gn", "gn launch", "plain, gn launch")
GN_TABLE = ((256, 1, 256), (512, 2, 256), (1024, 4, 256), (2048, 8, 256), (4096, 8, 512), (8192, 8, 1024))   # launch_reduce_gn
FIELDS = ("route", "npt", "nblk", "ks", "safe", "reduce", "nv", "nt")                                         # vf_conv_fwd_plan's out[8]


def check_env(environ=None):
    """The library reads these knobs once per process; a plan under one of them is not the one restated here."""
    bad = [k for k in ENV if k in (os.environ if environ is None else environ)]
    if bad:
        raise RuntimeError(f"{', '.join(bad)} set: the conv plan tests describe the default plan only; unset them")


check_env()

rup, cdiv = wp.rup, wp.cdiv


# ------------------------------------------------------------------------------------------------ the planners
def square_pow2(H, W):
    return H == W and W in (8, 16, 32, 64, 128)


def fwd_specialised(KS, H, W, mode):
    """csrc/conv.hip: the (KS, map, mode) table of conv_mfma_kernel."""
    return square_pow2(H, W) and (KS, mode) in SPEC_MAPS and W in SPEC_MAPS[KS, mode]


def views_per_tile(HW, npt):
    """Geo::IM: whole images per tile where an image has fewer pixels than the tile."""
    return 1 if HW >= 64 * npt else 64 * npt // HW


def conv_blocks(S, CoutP, HW, npt):
    im = views_per_tile(HW, npt)
    ntiles = S * (HW // (64 * npt)) if im == 1 else cdiv(S, im)
    return ntiles * (CoutP // 64)


def choose_ksplit(nblk, nch):
    """The largest split that still gives every workgroup a CU in one round, at most 16, at most one chunk each."""
    k = np.maximum(np.minimum(np.minimum(KSPLIT_WGS // np.maximum(nblk, 1), 16), nch), 1)
    return np.where((nblk >= KSPLIT_WGS) | (nch < 2), 1, k)


def reduce_gn_variant(n4g):
    """launch_reduce_gn's table -> (NV, NT), (0, 0) where a (view, group) of n4g float4 is too large."""
    nv, nt = np.zeros_like(n4g), np.zeros_like(n4g)
    for lim, v, t in reversed(GN_TABLE):
        nv, nt = np.where(n4g <= lim, v, nv), np.where(n4g <= lim, t, nt)
    return nv, nt


def conv1x1_halves(S, Cin, Cout, HW):
    """vfi_conv1x1_halves, natural policy: 2 = 128-channel workgroups, 1 = 64-channel ones, 0 = not taken."""
    nct, ptiles = cdiv(Cout, 64), cdiv(S * HW, 128)
    two = (Cin >= 256) & (nct % 2 == 0) & (ptiles * (nct // 2) >= 512)
    one = (Cin >= 128) & (nct >= 4) & (ptiles * nct >= 192)
    return np.where(two, 2, np.where(one, 1, 0))


def conv1x1_supported(S, Cin, Cout, HW, C1=0):
    """vfi_conv1x1_supported, natural policy (C1 / C1o already satisfy the entry's rules)."""
    npx = S * HW
    widest = np.maximum(C1, Cin - C1) if C1 else Cin
    ok = (Cin % 32 == 0) & (HW >= 64) & ((HW & (HW - 1)) == 0) & (npx >= 128) & (npx % 4 == 0) & (S * widest * HW * 4 < 2 ** 32)
    return ok & (conv1x1_halves(S, Cin, Cout, HW) != 0)


def any_plan(S, Cin, Cout, H, W, KS):
    """fwd_plan (csrc/conv_any.hip) -> (npt, nblk, ks before the workspace rules)."""
    npix, nco = S * H * W, cdiv(Cout, 64)
    npt = np.where(cdiv(npix, 128) * nco >= CONV_MIN_WGS, 2, 1)
    nblk = cdiv(npix, 64 * npt) * nco
    ck = 8 if KS == 3 else 32
    nch = cdiv(Cin, ck)
    nbk = cdiv(npix, 128) * nco if square_pow2(H, W) else nblk     # (square power-of-two map: the specialised price)
    k = np.maximum(np.minimum(np.minimum(256 // np.maximum(nbk, 1), 16), nch), 1)
    return npt, nblk, np.where((nbk < 256) & (nch >= 2), k, 1)


def ws_floats(S, Cin, Cout, H, W, KS):
    """vf_conv_fwd_ws_floats: 128-pixel tiles, no mode."""
    ck = 8 if KS == 3 else 32
    if square_pow2(H, W):
        ks = choose_ksplit(cdiv(S * H * W, 128) * (rup(Cout, 64) // 64), rup(Cin, ck) // ck)
    else:
        ks = any_plan(S, Cin, Cout, H, W, KS)[2]
    return np.where(ks > 1, ks * S * Cout * H * W, 0)


def plan_arrays(S, Cin, Cout, H, W, KS, mode, C1=0, C1o=0, gn=0, ws="priced"):
    """conv_fwd_plan.  C1 / C1o: 0, or the first part of a concatenated input / split output; gn: GroupNorm groups of
    vf_conv_fwd_gn or 0; ws: None (no workspace), "priced" (vf_conv_fwd_ws_floats of the shape) or a number of floats.
    -> dict of FIELDS (what the library reports) and of the quantities the classes need."""
    S, Cin, Cout = (np.asarray(v, dtype=np.int64) for v in (S, Cin, Cout))
    HW, ck = H * W, 8 if KS == 3 else 32
    nch = rup(Cin, ck) // ck
    out_floats = S * Cout * HW
    need = ws_floats(S, Cin, Cout, H, W, KS)
    have = np.zeros_like(need) if ws is None else (need if isinstance(ws, str) else np.asarray(ws, dtype=np.int64) + 0 * need)
    has_ws = ws is not None
    zero = 0 * (S + Cin + Cout)
    if not fwd_specialised(KS, H, W, mode):
        npt, nblk, ks0 = any_plan(S, Cin, Cout, H, W, KS)
        ks = ks0 if (has_ws and not C1o and mode != 4) else 1 + zero
        ks = np.maximum(np.minimum(ks, have // out_floats), 1)
        red = np.where(ks > 1, RED_PLAIN_GN_LAUNCH if gn else RED_PLAIN, RED_GN_LAUNCH if gn else RED_NONE)
        d = dict(route=ANY + zero, npt=npt + zero, nblk=nblk + zero, ks=ks + zero, safe=zero, reduce=red + zero, nv=zero, nt=zero)
        d.update(ks0=ks0 + zero, im=zero + 1, half=zero != 0)
    else:
        CoutP = rup(Cout, 64)
        npt = np.where(conv_blocks(S, CoutP, HW, 2) < CONV_MIN_WGS, 1, 2) if HW <= 256 else 2 + zero
        nblk = np.where(npt == 1, conv_blocks(S, CoutP, HW, 1), conv_blocks(S, CoutP, HW, 2))
        im = np.where(npt == 1, views_per_tile(HW, 1), views_per_tile(HW, 2))
        ks0 = choose_ksplit(nblk, nch)
        ks = ks0 if (has_ws and not C1o and mode != 4) else 1 + zero
        ks = np.maximum(np.minimum(ks, have // out_floats), 1)
        half = (im > 1) & (S % im != 0)
        safe = (Cin % 32 == 0) & ~half if KS == 1 else zero != 0
        nv, nt = reduce_gn_variant((Cout // gn) * HW // 4) if gn else (zero, zero)
        if gn:
            red = np.where(ks > 1, np.where(nv > 0, RED_GN, RED_PLAIN_GN_LAUNCH), RED_GN_LAUNCH)
            nv, nt = np.where(red == RED_GN, nv, 0), np.where(red == RED_GN, nt, 0)
        else:
            red = np.where(ks > 1, RED_PLAIN, RED_NONE)
        d = dict(route=MFMA + zero, npt=npt + zero, nblk=nblk + zero, ks=ks + zero, safe=safe.astype(np.int64) + zero,
                 reduce=red + zero, nv=nv + zero, nt=nt + zero, ks0=ks0 + zero, im=im + zero, half=half | (zero != 0))
        if KS == 1 and not gn:         # training-size grids: the dedicated 1x1 kernel
            h = conv1x1_halves(S, Cin, Cout, HW)
            sup = conv1x1_supported(S, Cin, Cout, HW, C1)
            grid = cdiv(S * HW, 128) * np.where(h == 2, cdiv(cdiv(Cout, 64), 2), cdiv(Cout, 64))
            for k, v in dict(route=np.where(h == 2, ONE128, ONE64), npt=2, nblk=grid, ks=1, safe=0, reduce=RED_NONE, nv=0, nt=0,
                             ks0=1, im=1).items():
                d[k] = np.where(sup, v, d[k])
            d["half"] = d["half"] & ~sup
    d.update(nch=nch + zero, need=need + zero, pks=np.where(need > 0, need // out_floats, 1) + zero, out_floats=out_floats + zero)
    return d


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "S Cin Cout H W KS mode C1 C1o gn store_y why")


def mk(S, Cin, Cout, H, W, KS, mode, C1=0, C1o=0, gn=0, store_y=1, why=""):
    return Case(int(S), int(Cin), int(Cout), int(H), int(W), int(KS), int(mode), int(C1), int(C1o), int(gn), int(store_y), why)


def case_id(c):
    return (f"{c.H}x{c.W}-k{c.KS}m{c.mode}-S{c.S}-{c.Cin}x{c.Cout}" + (f"-cat{c.C1}" if c.C1 else "")
            + (f"-split{c.C1o}" if c.C1o else "") + (f"-gn{c.gn}{'y' if c.store_y else ''}" if c.gn else ""))


def cost(c):
    return c.S * c.H * c.W * c.Cin * c.Cout * c.KS * c.KS


def entry(c):
    return ("vf_conv1x1_cat_fwd" if c.C1 else "vf_conv1x1_cat_dgrad" if c.C1o else "vf_conv_fwd_gn" if c.gn else "vf_conv_fwd")


def plan(c, ws="priced"):
    """The plan of case c's launch as plain Python values (ws as in plan_arrays)."""
    d = plan_arrays(c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode, c.C1, c.C1o, c.gn, ws)
    return {k: (bool(v) if np.asarray(v).dtype == bool else int(v)) for k, v in d.items()}


def fields(d):
    return [d[k] for k in FIELDS]


def chunk_ranges(nch, ks):
    """Per split the chunk range [begin, end) of conv_mfma_kernel / conv_any_kernel."""
    return [(s * nch // ks, (s + 1) * nch // ks) for s in range(ks)]


def _ksb(ks):
    """ks bucket: 1 | 2-8 (one batch of the reduce) | 9-15 (a partly filled second batch) | 16."""
    return np.select([ks == 1, ks <= 8, ks <= 15], [0, 1, 2], 3)


KSB = ("1", "2-8", "9-15", "16")
PRICING = ("not priced", "as priced", "priced, fewer taken", "priced, one taken")


def _pricing(ks, pks):
    return np.select([pks == 1, ks == pks, ks > 1], [0, 1, 2], 3)


def cat_kind(c, d):
    """Where the concatenation boundary C1 falls in the K split: "unsplit" | "on a split boundary" | "inside a split"."""
    if d["ks"] == 1:
        return "unsplit"
    ck = 32
    return "on a split boundary" if c.C1 // ck in {b for b, _ in chunk_ranges(d["nch"], d["ks"])} else "inside a split"


def one_edge(S, Cin, Cout, HW):
    """The 1x1 route's three thresholds per variant (vfi_conv1x1_halves): the code of the threshold a shape stands next
    to, on either side -- the shape takes the variant and one step down in that quantity alone would lose it ("+"), or
    it misses the variant by that quantity alone and by one step ("-").  0: none.  Codes index ONE_EDGES."""
    S, Cin, Cout = (np.asarray(v, dtype=np.int64) for v in (S, Cin, Cout))
    nct, pt = cdiv(Cout, 64), cdiv(S * HW, 128)
    sup = (Cin % 32 == 0) & (HW >= 64) & (S * HW >= 128) & (S * HW % 4 == 0) & (S * Cin * HW * 4 < 2 ** 32)
    two = (Cin >= 256) & (nct % 2 == 0) & (pt * (nct // 2) >= 512)
    one = (Cin >= 128) & (nct >= 4) & (pt * nct >= 192) & ~two
    t2, t1 = pt * (nct // 2), pt * nct
    conds = [two & (Cin == 256), ~two & (Cin == 224) & (nct % 2 == 0) & (t2 >= 512),
             two & ((pt - 1) * (nct // 2) < 512), (Cin >= 256) & (nct % 2 == 0) & (t2 < 512) & ((pt + 1) * (nct // 2) >= 512),
             two & (nct >= 2), (Cin >= 256) & (nct % 2 == 1) & (t2 >= 512),
             one & (Cin == 128), ~two & (Cin == 96) & (nct >= 4) & (t1 >= 192),
             one & (nct == 4), ~two & (Cin >= 128) & (nct == 3) & (t1 >= 192),
             one & ((pt - 1) * nct < 192), ~two & (Cin >= 128) & (nct >= 4) & (t1 < 192) & ((pt + 1) * nct >= 192)]
    return [c & sup for c in conds]


ONE_EDGES = ("<2> Cin = 256 (+)", "<2> Cin = 224 (-)", "<2> first grid of 512 column tiles (+)", "<2> last grid below 512 (-)",
             "<2> even number of 64-channel tiles (+)", "<2> odd number of 64-channel tiles (-)",
             "<1> Cin = 128 (+)", "<1> Cin = 96 (-)", "<1> four 64-channel tiles (+)", "<1> three 64-channel tiles (-)",
             "<1> first grid of 192 tiles (+)", "<1> last grid below 192 (-)")


def _reduce_key(c, d):
    if d["reduce"] == RED_NONE:
        return None
    if d["reduce"] == RED_PLAIN:
        whole = (d["out_floats"] // 4) % 256 == 0
        return ("reduce plain", ROUTES[d["route"]], "whole" if whole else "ragged", "second batch" if d["ks"] > 8 else "one batch")
    if d["reduce"] == RED_GN:
        n4g, kb = (c.Cout // c.gn) * c.H * c.W // 4, max(8 // d["nv"], 1)
        return ("reduce+gn", d["nv"], d["nt"], "fills" if n4g == d["nv"] * d["nt"] else "clamped lanes",
                "whole batches" if d["ks"] % kb == 0 else "partly filled batch", "store_y" if c.store_y else "no y")
    return ("gn fallback", RED_NAMES[d["reduce"]], ROUTES[d["route"]])


def class_keys(c, d=None):
    """The coverage keys of case c's launch at the priced workspace."""
    d = plan(c) if d is None else d
    r = d["route"]
    ck = 8 if c.KS == 3 else 32
    keys = []
    if r == MFMA:
        keys.append(("tile", c.KS, c.W, c.mode, d["npt"], d["im"], "half-empty last tile" if d["half"] else "whole tiles"))
        keys.append(("split", c.KS, c.mode, KSB[int(_ksb(d["ks"]))], "uneven" if d["nch"] % d["ks"] else "even",
                     PRICING[int(_pricing(d["ks"], d["pks"]))], "half-empty last tile" if d["half"] else "whole tiles"))
        keys.append(("pad", c.KS, "Cin padded" if c.Cin % ck else "Cin whole", "Cout padded" if c.Cout % 64 else "Cout whole",
                     "Cout < 32" if c.Cout < 32 else "Cout >= 32"))
        if c.KS == 1:
            keys.append(("safe", "SAFE" if d["safe"] else "guarded", "Cin % 32" if c.Cin % 32 else "", "half" if d["half"] else ""))
    elif r == ANY:
        keys.append(("any", c.H, c.W, c.KS, c.mode, d["npt"], KSB[int(_ksb(d["ks"]))],
                     "partly filled last tile" if c.S * c.H * c.W % (64 * d["npt"]) else "whole tiles"))
    if c.KS == 1 and r != ANY and not c.gn and not c.C1 and not c.C1o:
        e = one_edge(c.S, c.Cin, c.Cout, c.H * c.W)
        keys += [("1x1 route", ROUTES[r], ONE_EDGES[i]) for i, v in enumerate(e) if bool(v)]
    if r in (ONE64, ONE128):
        keys.append(("1x1 kernel", ROUTES[r], c.W, "partly filled last tile" if c.S * c.H * c.W % 128 else "whole tiles"))
    if c.C1:
        keys.append(("cat", ROUTES[r], cat_kind(c, d), "second part % 32" if (c.Cin - c.C1) % 32 else "second part whole"))
    if c.C1o:
        keys.append(("split output", ROUTES[r]))
    if c.mode == 4 and d["ks0"] > 1:
        keys.append(("mode 4 with a priced workspace", ROUTES[r]))
    rk = _reduce_key(c, d)
    return keys + ([rk] if rk else [])


# hand-written cases
SPECIALS = (
    mk(3, 128, 64, 8, 8, 3, 4, why="mode 4 with the priced workspace on a specialised map: choose_ksplit = 16, the epilogue has no partial-sum form"),
    mk(2, 64, 64, 6, 10, 3, 4, why="mode 4 with the priced workspace on the general kernel"),
    # (Cin = 96 keeps the 192-channel output tiles of these four under the cap; the plan depends on Cin through nch only)
    mk(22, 96, 192, 16, 16, 3, 0, why="S = 22: 132 tiles of 128 pixels but 264 of 64 (the price is 0: 256 / 132 = 1)"),
    mk(22, 96, 192, 16, 16, 3, 0, gn=GROUPS, why="S = 22 with GroupNorm: GroupNorm launch behind an unsplit conv"),
    mk(21, 96, 192, 16, 16, 3, 0, why="S = 21: priced for 126 tiles of 128 pixels (ks = 2), 252 tiles of 64 taken (ks = 1)"),
    mk(21, 96, 192, 16, 16, 3, 0, gn=GROUPS, why="S = 21 with GroupNorm: ops decides 'fused' from the price, the launch falls back"),
    mk(1, 64, 64, 128, 128, 3, 0, gn=GROUPS, store_y=0, why="64 -> 64 on 128 x 128 at S = 1: reduce + GroupNorm variant (8, 1024)"),
    # (with 32 groups no split launch has a group above 8192 float4: 64 x 64 needs Cout >= 288, i.e. 160 workgroups)
    mk(1, 32, 128, 64, 64, 3, 0, gn=8, why="8 groups of 16 channels on 64 x 64: 16384 float4 a group, plain reduce then a GroupNorm launch"),
    mk(3, 96, 96, 8, 8, 3, 0, gn=GROUPS, store_y=0, why="cpg = 3: 48 float4 on 256 lanes (clamped lanes), half-empty 8 x 8 tile"),
    mk(2, 320, 320, 8, 8, 3, 0, gn=GROUPS, why="cpg = 10: 160 float4 on 256 lanes"),
    mk(5, 128, 64, 6, 10, 1, 0, C1=64, why="general kernel, 1x1 on a concatenation"),
    mk(5, 64, 128, 6, 10, 1, 0, C1o=64, why="general kernel, 1x1 with a split output"),
    # the bench step's stride-2 and 1x1 layers at S = 96, channels scaled down to the cap with the tile plan unchanged
    mk(96, 64, 16, 32, 32, 3, 1, why="bench stride-2 64 -> 64 @32 at S = 96 (Cout scaled)"),
    mk(96, 128, 16, 16, 16, 3, 1, why="bench stride-2 128 -> 128 @16 at S = 96 (Cout scaled)"),
    mk(96, 192, 32, 8, 8, 3, 1, why="bench stride-2 192 -> 192 @8 at S = 96 (Cout scaled)"),
    mk(96, 16, 64, 32, 32, 3, 4, why="bench stride-2 dgrad 64 -> 64 @32 at S = 96 (K scaled)"),
    mk(96, 64, 128, 32, 32, 1, 0, why="bench 1x1 64 -> 128 @32 at S = 96 (conv_mfma: K too short for conv1x1)"),
    mk(96, 128, 192, 16, 16, 1, 0, why="bench 1x1 128 -> 192 @16 at S = 96 (three tiles: conv_mfma)"),
    mk(96, 192, 128, 16, 16, 1, 0, why="bench 1x1 dgrad 192 -> 128 @16 at S = 96"),
    mk(96, 128, 64, 32, 32, 1, 0, why="bench 1x1 dgrad 128 -> 64 @32 at S = 96"),
)


def _grid():
    S = np.arange(1, S_MAX + 1, dtype=np.int64)[:, None, None]
    Ci = np.array(CHANNELS, dtype=np.int64)[None, :, None]
    Co = np.array(CHANNELS, dtype=np.int64)[None, None, :]
    return S, Ci, Co


def rows():
    """(H, W, KS, mode) of the whole sweep: the launch tables and ANY_SHAPES."""
    return [(W, W, KS, mode) for (KS, mode), maps in sorted(SPEC_MAPS.items()) for W in maps] + list(ANY_SHAPES)


def _encode(attrs):
    """Mixed-radix code of small non-negative integer attribute arrays."""
    key = 0
    for a in attrs:
        a = np.asarray(a).astype(np.int64)
        key = key * (int(a.max()) + 1) + a
    return key


def _sweep_keys(H, W, KS, mode, gn=0, capped=True):
    """Integer class codes over the grid, one array per key family of class_keys (the representatives are re-classified by
    class_keys itself: the codes only have to separate what it separates) -> [(codes, valid)]."""
    S, Ci, Co = _grid()
    d = plan_arrays(S, Ci, Co, H, W, KS, mode, gn=gn)
    ck = 8 if KS == 3 else 32
    valid = (S * H * W * Ci * Co * KS * KS <= CAP_MACS) | (not capped)
    out = []
    if gn:
        valid = valid & (Co % gn == 0)
        n4g = (Co // gn) * H * W // 4
        kb = np.maximum(8 // np.maximum(d["nv"], 1), 1)
        out.append((_encode([d["reduce"], d["nv"], d["nt"], n4g == d["nv"] * d["nt"], d["ks"] % kb == 0, d["route"]]), valid))
        return out
    mf, an = d["route"] == MFMA, d["route"] == ANY
    out.append((_encode([d["npt"], d["im"], d["half"]]), valid & mf))
    out.append((_encode([_ksb(d["ks"]), d["nch"] % d["ks"] != 0, _pricing(d["ks"], d["pks"]), d["half"]]), valid & mf))
    out.append((_encode([Ci % ck != 0, Co % 64 != 0, Co < 32]), valid & mf))
    if KS == 1:
        out.append((_encode([d["safe"], Ci % 32 != 0, d["half"]]), valid & mf))
        out.append((_encode([d["route"], S * H * W % 128 != 0]), valid & ~mf & ~an))
        if not an.any():
            for e in one_edge(S, Ci, Co, H * W):
                out.append((_encode([d["route"]]), valid & e))
    out.append((_encode([d["npt"], _ksb(d["ks"]), S * H * W % (64 * d["npt"]) != 0]), valid & an))
    out.append((_encode([d["reduce"], (d["out_floats"] // 4) % 256 == 0, d["ks"] > 8, d["route"]]), valid & (d["reduce"] == RED_PLAIN)))
    return out


def _cat_sweep():
    """Concatenated input / split output (1x1): a sweep small enough to classify case by case."""
    for W in SPEC_MAPS[1, 0]:
        for S in (2, 3, 6, 12, 96):
            for Cin, Cout in ((96, 64), (128, 64), (160, 64), (192, 128), (288, 64), (320, 192), (576, 192), (640, 320), (960, 320),
                              (320, 256), (384, 256), (200, 64), (328, 128), (256, 128)):
                for C1 in (32, 64, 96, 128, 192, 256, 320):
                    if 0 < C1 < Cin:
                        yield mk(S, Cin, Cout, W, W, 1, 0, C1=C1)
                        if C1 % 64 == 0:
                            yield mk(S, Cout, Cin, W, W, 1, 0, C1o=C1)


def _best(capped):
    """{class key: (sort key, cheapest case)} over the domain and the concatenation sweep."""
    best = {}

    def offer(c):
        sk = (c.S < 2, cost(c), c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode, c.C1, c.C1o, c.gn, -c.store_y)
        for k in class_keys(c):
            if k not in best or sk < best[k][0]:
                best[k] = (sk, c)

    for H, W, KS, mode in rows():
        for gn in ((0, GROUPS) if mode in (0, 2) else (0,)):
            for codes, valid in _sweep_keys(H, W, KS, mode, gn, capped):
                if valid.any():
                    for s, ci, co in wp._cheapest(np.where(valid, codes, 0), valid).values():
                        for sy in ((1, 0) if gn else (1,)):
                            offer(mk(s, ci, co, H, W, KS, mode, gn=gn, store_y=sy))
    for c in _cat_sweep():
        if not capped or cost(c) <= CAP_MACS:
            offer(c)
    return best


@functools.lru_cache(maxsize=None)
def _enumerate():
    """Per class key its cheapest case over the domain (two or more views first, then the fewest multiply-adds), the
    concatenation / split-output classes over a small sweep of their own, and SPECIALS."""
    found = collections.OrderedDict()
    for c in SPECIALS:
        found.setdefault(c[:-1], []).append(c.why)
    for k, (_, c) in sorted(_best(True).items(), key=lambda kv: str(kv[0])):
        found.setdefault(c[:-1], []).append("class " + " ".join(str(v) for v in k))
    return tuple(Case(*k, "; ".join(dict.fromkeys(v))) for k, v in found.items())


def cases():
    return list(_enumerate())


@functools.lru_cache(maxsize=None)
def _over_cap():
    have = case_classes()
    return {k: (c, cost(c)) for k, (_, c) in _best(False).items() if k not in have}


def over_cap_classes():
    """{class key: (cheapest case, multiply-adds)} of the classes whose cheapest representative anywhere in the domain
    costs more than CAP_MACS: named, not run (conv1x1_kernel<2> needs 512 column tiles of 128 pixels x 128 channels at
    Cin >= 256: 2.1e9 multiply-adds at the least)."""
    return dict(_over_cap())


def case_classes():
    return {k for c in cases() for k in class_keys(c)}


def model_layers():
    """(Cin, Cout, H, KS, mode, C1 | 0) of every conv of the SMALL and TINY networks (tests/test_wgrad_plan_host.py)."""
    from test_wgrad_plan_host import _model_layers
    return _model_layers()


@functools.lru_cache(maxsize=None)
def covered_classes():
    """{class key: the first launch that reaches it} over what the SMALL and TINY networks launch at S = 1 .. 368 through
    vf_conv_fwd and its kin -- every layer forward (with the GroupNorm of vf_conv_fwd_gn where a 3x3 layer can have one)
    and in dgrad direction (Cin <-> Cout; stride 2: mode 4 on the dY map; Upsample: mode 0 on the output map; a
    concatenated input forward = a split output backward), whether or not the policy sends the layer here at that S."""
    reached = {}
    for Cin, Cout, H, KS, mode, C1 in model_layers():
        launches = [(Cin, Cout, H, KS, mode, 0, 0, 0), (Cout, Cin, H, KS, 4 if mode == 1 else 0, 0, 0, 0)]
        if KS == 3 and mode in (0, 2) and Cout % GROUPS == 0:
            launches.append((Cin, Cout, H, KS, mode, 0, 0, GROUPS))
        if C1 and C1 % 64 == 0:
            launches += [(Cin, Cout, H, KS, mode, C1, 0, 0), (Cout, Cin, H, KS, 0, 0, C1, 0)]
        for ci, co, h, ks, m, c1, c1o, gn in launches:
            # class_keys depends on S through the plan, the fill of the last tile / reduce workgroup and the 1x1 edges
            # only: one representative S per distinct combination of those
            S = np.arange(1, S_MAX + 1, dtype=np.int64)
            d = plan_arrays(S, ci, co, h, h, ks, m, c1, c1o, gn)
            attrs = [d[k] for k in ("route", "npt", "ks", "safe", "reduce", "nv", "nt", "ks0", "pks", "half")]
            attrs += [S * h * h % 128 != 0, S * h * h % (64 * d["npt"]) != 0, (d["out_floats"] // 4) % 256 == 0]
            attrs += one_edge(S, ci, co, h * h)
            _, first = np.unique(_encode(attrs), return_index=True)
            for i in sorted(first.tolist()):
                for sy in ((1, 0) if gn else (1,)):
                    c = mk(S[i], ci, co, h, h, ks, m, C1=c1, C1o=c1o, gn=gn, store_y=sy)
                    for k in class_keys(c):
                        reached.setdefault(k, case_id(c))
    return reached


def hygiene_cases():
    """One case per (route, reduce kind, ks bucket, store_y, split output, mode 4): the cheapest."""
    pick = {}
    for c in sorted(cases(), key=lambda c: (cost(c), case_id(c))):
        d = plan(c)
        pick.setdefault((d["route"], d["reduce"], int(_ksb(d["ks"])), c.store_y, bool(c.C1o), c.mode == 4 and d["ks0"] > 1, d["half"]), c)
    return list(pick.values())


def clip_cases():
    """Per (route, reduce kind) with a split the cheapest case with ks >= 4, and the one with the largest ks."""
    out = {}
    for c in sorted(cases(), key=lambda c: (cost(c), case_id(c))):
        d = plan(c)
        if d["ks"] >= 4:
            out.setdefault((d["route"], d["reduce"], "cheapest"), c)
            k = (d["route"], d["reduce"], "widest")
            if k not in out or d["ks"] > plan(out[k])["ks"]:
                out[k] = c
    return list(dict.fromkeys(out.values()))


# ------------------------------------------------------------------------------------------------ inputs and references
def in_size(c):
    return {0: (c.H, c.W), 1: (2 * c.H, 2 * c.W), 2: (c.H // 2, c.W // 2), 4: (c.H, c.W)}[c.mode]


def out_size(c):
    return (2 * c.H, 2 * c.W) if c.mode == 4 else (c.H, c.W)


def weight_shape(c):
    """The layer's OIHW parameter: mode 4 runs the stride-2 layer Cout -> Cin backwards (its weight is (Cin, Cout, 3, 3))."""
    return (c.Cin, c.Cout, c.KS, c.KS) if c.mode == 4 else (c.Cout, c.Cin, c.KS, c.KS)


def inputs(c):
    """-> dict(x, w (OIHW of the layer), bias, vbias, res, gamma, beta), float32 on the CPU, seeded."""
    Hi, Wi = in_size(c)
    Ho, Wo = out_size(c)
    return dict(x=wp.rnd(c.S, c.Cin, Hi, Wi, seed=7), w=wp.rnd(*weight_shape(c), seed=5) / math.sqrt(c.Cin * c.KS * c.KS),
                bias=wp.rnd(c.Cout, seed=6) * 0.1, vbias=wp.rnd(c.S, c.Cout, seed=8) * 0.3, res=wp.rnd(c.S, c.Cout, Ho, Wo, seed=9) * 0.5,
                gamma=1 + 0.3 * wp.rnd(c.Cout, seed=11), beta=0.2 * wp.rnd(c.Cout, seed=12))


def operands(c, full):
    """Which epilogue operands a call has: (bias, vbias, res).  The cat forward takes a bias only, the cat dgrad and a bare
    call nothing, mode 4 a residual only."""
    if c.C1o or not full:
        return (False, False, False)
    if c.C1:
        return (True, False, False)
    if c.mode == 4:
        return (False, False, True)
    return (True, True, True)


def _conv(x, w, c):
    if c.mode == 4:
        return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    if c.mode == 2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return F.conv2d(x, w, stride=2 if c.mode == 1 else 1, padding=c.KS // 2)


def _epilogue(y, t, c, full, dt):
    b, v, r = operands(c, full)
    if r:
        y = y + t["res"].to(dt)
    if b or v:
        add = (t["bias"].to(dt)[None, :] if b else 0) + (t["vbias"].to(dt) if v else 0)
        y = y + add[:, :, None, None]
    return y


def gn_f(y, t, c, dt):
    if dt == torch.float64:
        import cond_ref as cr
        return cr.gn_forward_f64(y, t["gamma"], t["beta"], True, c.gn)
    return F.silu(F.group_norm(y, c.gn, t["gamma"], t["beta"], 1e-5))


def conv_core(t, c, dtype):
    """F.conv2d (conv_transpose2d for mode 4) in `dtype` on the CPU, no epilogue: the expensive part, computed once."""
    return _conv(t["x"].to(dtype), t["w"].to(dtype), c)


def conv_ref(t, c, dtype, full=True, core=None):
    """conv_core + the call's epilogue operands (full) or none (bare) -> [y, (gn(y))]."""
    y = _epilogue(conv_core(t, c, dtype) if core is None else core, t, c, full, dtype)
    return [y] + ([gn_f(y, t, c, dtype)] if c.gn else [])


# ------------------------------------------------------------------------------------------------ the split model
MUTANTS = ("drop_last_chunk", "ceil_ranges", "skip_second_batch", "cat_wrong_source", "half_tile_view0", "gn_clamped_lanes")


def batch_size(d):
    """Partials per batch of the reduce: eight, or 8 / NV in the reduce + GroupNorm kernel."""
    return max(8 // d["nv"], 1) if d["reduce"] == RED_GN else 8


def mutant_applies(c, d, m):
    if d["route"] not in (MFMA, ANY):
        return m == "cat_wrong_source" and bool(c.C1)
    if m in ("drop_last_chunk", "ceil_ranges"):
        return d["ks"] > 1 and d["nch"] % d["ks"] != 0
    if m == "skip_second_batch":
        return d["ks"] > batch_size(d) and d["route"] == MFMA
    if m == "cat_wrong_source":
        return bool(c.C1)
    if m == "half_tile_view0":
        return d["half"] and c.S > 1
    if m == "gn_clamped_lanes":
        return d["reduce"] == RED_GN and (c.Cout // c.gn) * c.H * c.W // 4 < d["nv"] * d["nt"]
    raise KeyError(m)


def conv_split(t, c, d, mutate=None, full=True):
    """The split decomposition in float32 on the CPU: one partial per K range over exactly that range's channels, the
    partials added in index order, batch by batch (eight, or 8 / NV, independent loads: the sum is sequential within and
    across batches), then residual and bias as the reduce kernel adds them; reduce + GroupNorm: two-pass statistics over
    the group's own float4 -> [y, (gn(y))].  mutate, one of MUTANTS:
      drop_last_chunk    the last chunk of the longest range is not multiplied
      ceil_ranges        range ends by ceiling instead of floor: neighbouring ranges overlap by a chunk
      skip_second_batch  the first partial of the second batch is not added
      cat_wrong_source   the chunk at the concatenation boundary is read from the first source's last 32 channels
      half_tile_view0    the view of the half-empty last tile is computed from view 0's input
      gn_clamped_lanes   the lanes clamped onto the group's last float4 are counted in the mean"""
    assert mutate is None or (mutate in MUTANTS and mutant_applies(c, d, mutate))
    x, w = t["x"].clone(), t["w"]
    ck = 8 if c.KS == 3 else 32
    if mutate == "cat_wrong_source":
        x[:, c.C1:min(c.C1 + 32, c.Cin)] = x[:, c.C1 - 32:c.C1][:, :min(32, c.Cin - c.C1)]
    if mutate == "half_tile_view0":
        x[c.S - 1] = x[0]
    ks = d["ks"] if d["route"] in (MFMA, ANY) else 1
    ranges = chunk_ranges(d["nch"], ks)
    if mutate == "ceil_ranges":
        ranges = [(b, -(-(s + 1) * d["nch"] // ks)) for s, (b, _) in enumerate(ranges)]
    if mutate == "drop_last_chunk":
        s = max(range(ks), key=lambda i: (ranges[i][1] - ranges[i][0], i))
        ranges[s] = (ranges[s][0], ranges[s][1] - 1)
    kdim = 0 if c.mode == 4 else 1              # the K (input-channel) axis of the layer's OIHW parameter
    parts = []
    for b, e in ranges:
        lo, hi = b * ck, min(e * ck, c.Cin)
        parts.append(_conv(x[:, lo:hi], w.narrow(kdim, lo, hi - lo), c))
    skip = batch_size(d) if mutate == "skip_second_batch" else None
    v = torch.zeros_like(parts[0]) if ks > 1 else parts[0]
    if ks > 1:
        for k, p in enumerate(parts):
            if k != skip:
                v = v + p
    y = _epilogue(v, t, c, full, torch.float32)
    if not c.gn:
        return [y]
    if mutate != "gn_clamped_lanes":
        return [y, gn_f(y, t, c, torch.float32)]
    cpg = c.Cout // c.gn
    n4 = cpg * c.H * c.W // 4
    g = y.reshape(c.S, c.gn, -1)
    extra = d["nv"] * d["nt"] - n4                                  # lanes clamped onto the last float4
    mean = (g.sum(-1) + extra * g[:, :, -4:].sum(-1)) / (n4 * 4)
    var = ((g - mean[:, :, None]) ** 2).mean(-1)
    a = ((g - mean[:, :, None]) / torch.sqrt(var[:, :, None] + 1e-5)).reshape(y.shape)
    return [y, F.silu(a * t["gamma"][None, :, None, None] + t["beta"][None, :, None, None])]
