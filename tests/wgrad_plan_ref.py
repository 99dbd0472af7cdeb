"""The slab plans of the four weight-gradient launchers restated in pure Python -- launch_wgrad (csrc/conv.hip, "direct":
3x3 on square power-of-two maps), conv_wgrad_impl's KS == 1 branch ("1x1", also on a never-materialised concatenation),
launch_wino44_wgrad (csrc/winograd44.hip, "f44": F(4x4,3x3)) and vfi_conv_any_wgrad (csrc/conv_any.hip, "any": every
other geometry) -- with their *_ws_floats functions, the slab sums' trip structure (csrc/wgrad_reduce.h,
wino44_reduce_body), the plan-class enumeration behind tests/test_gpu_wgrad_plan.py, and the inputs / references /
CPU slab model its cases share.

A launch cuts its `units` (128-pixel tiles / 64-pixel steps / chunks of four 4x4 tiles / 16-pixel steps) into z slices
of `per` units, the last one `last` <= per units long; every slice writes one slab of partial dW, a second launch sums
the slabs in a fixed order.  The coverage keys of a launch are its plan class (plan_classes: one key per family, the 1x1
key in two halves) and the class of its slab sum (reduce_class); cases() holds the cheapest representative of every key
over the domain below, and a few hand-written layers (SPECIALS).

The arithmetic below works on Python ints and on numpy arrays alike: the enumeration evaluates the very functions that
tests/test_wgrad_plan_host.py pins to libvf_hip.so, on the whole domain at once.  Imports no GPU code."""
import collections
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

TOL_DW, TOL_DB = 1e-4, 2e-5          # the project's tolerances (tests/test_gpu_kernels.py)
NAMES = ("dW", "db", "db2")
CAP_MACS = 1e9                       # reference cost a case may have: S Hout Wout Cin Cout KS^2
ENV = ("VF_WINO_WGRAD_MIN_TILES",)
WINO_WGRAD_MIN_TILES = 256           # ops/state.py: the default use_winograd_wgrad() edge, S (H/2) (W/2) >= 256
TARGET_WGS = 512                     # WGRAD_TARGET_WGS

# the enumeration's domain
S_MAX = 368
CHANNELS = tuple(sorted({3, 6, 200, 576} | set(range(32, 961, 32))))
DIRECT_MAPS = {0: (8, 16, 32, 64, 128), 1: (8, 16, 32, 64), 2: (16, 32, 64, 128)}      # conv_wgrad_impl's VF_CASE table
ONE_MAPS = (8, 16, 32, 64, 128)
F44_MAPS, F44_MODES = (8, 16, 32, 64), (0, 2)                                           # vf_wino_wgrad_supported
# (H, W, KS, mode) of the general kernel: the shapes of tests/test_gpu_envelope_kernels.py (8 x 8 mode 2 = the 4 -> 8 Upsample)
ANY_SHAPES = ((24, 40, 3, 0), (6, 10, 3, 1), (12, 20, 3, 2), (5, 5, 1, 0), (5, 5, 3, 0), (8, 8, 3, 2))
FAMILIES = ("direct", "1x1", "f44", "any")
UNIT_PX = {"direct": 128, "1x1": 64, "f44": 64, "any": 16}
ENTRY = {"direct": "vf_conv_wgrad", "1x1": "vf_conv_wgrad", "f44": "vf_wino_wgrad", "any": "vf_conv_wgrad"}


def check_env(environ=None):
    """ops reads the policy override once per process; a route under it is not the one restated here."""
    bad = [k for k in ENV if k in (os.environ if environ is None else environ)]
    if bad:
        raise RuntimeError(f"{', '.join(bad)} set: the weight-gradient plan tests describe the default plan only; unset them")


check_env()


def rup(v, m):
    return (v + m - 1) // m * m


def cdiv(a, b):
    return (a + b - 1) // b


def _slices(units, z):
    """per = ceil(units / z), z recomputed: the last slice may be shorter."""
    per = cdiv(units, z)
    z = cdiv(units, per)
    return z, per, units - (z - 1) * per


def _clip(z, ws, slab, tail=0):
    """-> (z clipped to the slabs ws floats hold, launch accepted)."""
    if ws is None:
        return z, True
    zmax = np.maximum(ws - tail, 0) // slab
    return np.minimum(z, np.maximum(zmax, 1)), (ws >= slab + tail)


# ------------------------------------------------------------------------------------------------ the four planners
def wgrad1_tile(C):
    """128 unless the padding to 128 costs more than 20 %."""
    return np.where(5 * rup(C, 128) <= 6 * rup(C, 64), 128, 64)


def square_pow2(H, W):
    return H == W and W in (8, 16, 32, 64, 128)


def direct_specialised(KS, H, W, mode):
    """wgrad_specialised (csrc/conv.hip)."""
    if not square_pow2(H, W):
        return False
    return mode == 0 if KS == 1 else (KS == 3 and mode in DIRECT_MAPS and W in DIRECT_MAPS[mode])


def plan_direct(S, Cin, Cout, W, mode, ws=None):
    """launch_wgrad<3, log2 W, mode>: conv_wgrad_kernel<3, LOGW, MODE, BIG = mode != 1>."""
    big = mode != 1
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    im = 2 if W == 8 else 1                                   # images per 128-pixel tile
    units = cdiv(S, 2) if im == 2 else S * (W * W // 128)
    nco, nci = CoutP // 64, cdiv(CinQ, 64 if big else 32)
    slab = 9 * CoutP * CinQ
    z = np.minimum(np.maximum((256 if big else TARGET_WGS) // (nco * nci), 1), units)
    z, ok = _clip(z, ws, slab)
    z, per, last = _slices(units, z)
    return dict(variant="big" if big else "small", units=units, z=z, per=per, last=last, CoutP=CoutP, CinQ=CinQ,
                half=(S % 2 == 1) if im == 2 else S * 0 != 0, partial_step=S * 0 != 0, slab=slab, ok=ok, nt=9, tail=0,
                need=ws_conv(S, Cin, Cout, W, W, 3), nmain=cdiv(9 * Cout * Cin, 64))


def plan_1x1(S, Cin, Cout, W, ws=None):
    """conv_wgrad_impl, KS == 1: conv1x1_wgrad_kernel<tm, tn>."""
    tm, tn = wgrad1_tile(Cout), wgrad1_tile(Cin)
    CoutP, CinQ = rup(Cout, tm), rup(Cin, tn)
    units = S * (W * W // 64)
    slab = CoutP * CinQ
    z = np.maximum(np.minimum(TARGET_WGS // ((CoutP // tm) * (CinQ // tn)), units // 4), 1)
    z, ok = _clip(z, ws, slab)
    z, per, last = _slices(units, z)
    return dict(variant=(tm, tn), tm=tm, tn=tn, units=units, z=z, per=per, last=last, CoutP=CoutP, CinQ=CinQ, half=S * 0 != 0,
                partial_step=S * 0 != 0, slab=slab, ok=ok, nt=1, tail=0, need=ws_conv(S, Cin, Cout, W, W, 1),
                nmain=cdiv(Cout * Cin, 64))


def plan_f44(S, Cin, Cout, W, mode, ws=None):
    """launch_wino44_wgrad<log2 W, mode>: chunks of four 4x4 tiles; the per-slice dY sums sit behind the z slabs."""
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    units = S * ((W // 4) * (W // 4) // 4)
    slab, tail = 9 * CoutP * CinQ, 256 * CoutP
    z = np.minimum(np.maximum(256 // ((CoutP // 64) * (CinQ // 32)), 1), units)
    z, ok = _clip(z, ws, slab, tail)
    z, per, last = _slices(units, z)
    return dict(variant="f44", units=units, z=z, per=per, last=last, CoutP=CoutP, CinQ=CinQ, half=S * 0 != 0,
                partial_step=S * 0 != 0, slab=slab, ok=ok, nt=0, tail=tail, need=ws_f44(S, Cin, Cout, W, W),
                nmain=Cout * cdiv(Cin, 64))


def wgrad_slices(nco, Cin, npix, nsteps, sq, ws, slab):
    """csrc/conv_any.hip: ~512 workgroups over the (co, ci) tiles; on a square power-of-two map the specialised formula."""
    if sq:
        z = np.minimum(cdiv(512, nco * cdiv(Cin, 32)), cdiv(npix, 128))
    else:
        z = 512 // (nco * cdiv(Cin, 64))
    z = np.minimum(np.maximum(z, 1), nsteps)
    return z if ws is None else np.minimum(z, ws // slab)


def plan_any(S, Cin, Cout, H, W, KS, mode, ws=None):
    """vfi_conv_any_wgrad: 16-pixel steps, the last one partly filled when S H W % 16 != 0."""
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    npix = S * H * W
    units = cdiv(npix, 16)
    slab = KS * KS * CoutP * CinQ
    z = wgrad_slices(CoutP // 64, Cin, npix, units, square_pow2(H, W), ws, slab)
    ok = z >= 1
    z, per, last = _slices(units, np.maximum(z, 1))
    return dict(variant="sq" if square_pow2(H, W) else "free", units=units, z=z, per=per, last=last, CoutP=CoutP, CinQ=CinQ,
                half=S * 0 != 0, partial_step=npix % 16 != 0, slab=slab, ok=ok, nt=KS * KS, tail=0,
                need=ws_conv(S, Cin, Cout, H, W, KS), nmain=cdiv(KS * KS * Cout * Cin, 64))


# ------------------------------------------------------------------------------------------------ *_ws_floats
def ws_any(S, Cin, Cout, H, W, KS):
    """vfi_conv_any_wgrad_ws_floats."""
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    slab = KS * KS * CoutP * CinQ
    return wgrad_slices(CoutP // 64, Cin, S * H * W, cdiv(S * H * W, 16), square_pow2(H, W), None, slab) * slab


def ws_conv(S, Cin, Cout, H, W, KS):
    """vf_conv_wgrad_ws_floats.  The KS = 3 formula takes a CEILING over 32-channel ci tiles where launch_wgrad takes a
    floor over 64-channel ones (BIG) or a floor over 32-channel ones: it over-allocates by design, never under."""
    if not square_pow2(H, W):
        return ws_any(S, Cin, Cout, H, W, KS)
    if KS == 1:
        tm, tn = wgrad1_tile(Cout), wgrad1_tile(Cin)
        CoutP, CinQ = rup(Cout, tm), rup(Cin, tn)
        z = np.maximum(np.minimum(TARGET_WGS // ((CoutP // tm) * (CinQ // tn)), S * (H * W // 64) // 4), 1)
        return z * CoutP * CinQ
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    z = np.maximum(np.minimum(cdiv(TARGET_WGS, (CoutP // 64) * (CinQ // 32)), cdiv(S * H * W, 128)), 1)
    return z * KS * KS * CoutP * CinQ


def ws_f44(S, Cin, Cout, H, W):
    """vf_wino_wgrad_ws_floats."""
    CoutP, CinQ = rup(Cout, 64), rup(Cin, 32)
    z = np.minimum(np.maximum(256 // ((CoutP // 64) * (CinQ // 32)), 1), S * (H // 4) * (W // 4) // 4)
    return z * 9 * CoutP * CinQ + 256 * CoutP


def use_winograd_wgrad(S, H, W, KS, mode):
    """ops/policy.py at its defaults."""
    return KS == 3 and H == W and W in F44_MAPS and mode in F44_MODES and S * (H // 2) * (W // 2) >= WINO_WGRAD_MIN_TILES


# ------------------------------------------------------------------------------------------------ cases and classes
Case = collections.namedtuple("Case", "family S Cin Cout H W KS mode C1 db why")


def case_id(c):
    return (f"{c.family}-{c.H}x{c.W}-k{c.KS}m{c.mode}-S{c.S}-{c.Cin}x{c.Cout}" + (f"-cat{c.C1}" if c.C1 else "")
            + (f"-db{c.db}" if c.db else ""))


def cost(c):
    return c.S * c.H * c.W * c.Cin * c.Cout * c.KS * c.KS


def family_of(S, H, W, KS, mode):
    """The route of ops.conv2d / ops.conv1x1_cat at the default policy."""
    if use_winograd_wgrad(S, H, W, KS, mode):
        return "f44"
    if direct_specialised(KS, H, W, mode):
        return "direct" if KS == 3 else "1x1"
    return "any"


def _plain(d):
    one = lambda v: v if isinstance(v, str) else (bool(v) if np.asarray(v).dtype == bool else int(v))
    return {k: (tuple(one(e) for e in v) if isinstance(v, tuple) else one(v)) for k, v in d.items()}


def plan(c, ws=None):
    """The plan of case c's launch with ws floats of workspace (None: the preferred plan), as plain Python values."""
    if c.family == "direct":
        d = plan_direct(c.S, c.Cin, c.Cout, c.W, c.mode, ws)
    elif c.family == "1x1":
        d = plan_1x1(c.S, c.Cin, c.Cout, c.W, ws)
    elif c.family == "f44":
        d = plan_f44(c.S, c.Cin, c.Cout, c.W, c.mode, ws)
    else:
        d = plan_any(c.S, c.Cin, c.Cout, c.H, c.W, c.KS, c.mode, ws)
    d = _plain(d)
    d["family"] = c.family
    return d


def _bucket3(per):
    return np.minimum(per, 3)


def cat_class(C1, tn):
    """none | the split lies inside a 128-wide ci tile | on a tile edge (C1 % 64 == 0 is the ABI's precondition)."""
    return "none" if not C1 else ("inside" if C1 % int(tn) else "edge")


def plan_class(c, d=None):
    d = plan(c) if d is None else d
    short = d["last"] < d["per"]
    if c.family == "direct":
        return ("direct", c.mode, c.W, min(d["per"], 3), short, d["half"])
    if c.family == "1x1":
        return ("1x1", d["tm"], d["tn"], min(d["per"], 8), short, d["z"] == 1, d["CoutP"] > c.Cout, d["CinQ"] > c.Cin,
                cat_class(c.C1, d["tn"]))
    if c.family == "f44":
        return ("f44", c.W, c.mode, min(d["per"], 3), short, c.db >= 1, c.db >= 2)
    return ("any", c.KS, c.mode, square_pow2(c.H, c.W), min(d["per"], 3), short, d["partial_step"])


def plan_classes(c, d=None):
    """The coverage keys of a launch.  One per family -- except 1x1, whose key is kept in two halves, the tile half
    (tm, tn, Cout padded, Cin padded, concatenation) and the slice half (per, last slice short, z = 1): the slice loop of
    conv1x1_wgrad_kernel is one piece of code for all four tile variants, and the product of the two halves has no
    representative under CAP_MACS -- on 128 x 128 tiles a slice of six or more steps with z > 1 needs
    nsteps > 5 floor(512 / tiles), i.e. at least 5 * 512 * 64 * 96 * 96 = 1.5e9 multiply-adds."""
    cls = plan_class(c, d)
    if c.family != "1x1":
        return [cls]
    return [("1x1 tiles", cls[1], cls[2], cls[6], cls[7], cls[8]), ("1x1 slices", cls[3], cls[4], cls[5])]


NSLAB_BUCKETS = ("1", "2-4", "5-32", "33-63", "32k>=64", "other>=65")


def _nslab_bucket(n):
    return np.select([n == 1, n <= 4, n <= 32, n <= 63, n % 32 == 0], [0, 1, 2, 3, 4], 5)


def _ragged(nt, Cin, Cout):
    """The slab sum's last workgroup is partly filled: nt Cout Cin % 64 != 0 (F(4x4): 64 input channels a workgroup)."""
    return (Cin % 64 != 0) if nt == 0 else (nt * Cout * Cin % 64 != 0)


def reduce_class(c, d=None):
    d = plan(c) if d is None else d
    return ("reduce", d["nt"], NSLAB_BUCKETS[int(_nslab_bucket(d["z"]))], bool(_ragged(d["nt"], c.Cin, c.Cout)))


# hand-written cases: (reason, family, S, Cin, Cout, H, W, KS, mode, C1, db)
SPECIALS = (
    ("Cout = 6: below one co tile", "direct", 3, 64, 6, 16, 16, 3, 0, 0, 0),
    ("Cin = 6: below one ci tile", "direct", 3, 6, 64, 16, 16, 3, 0, 0, 0),
    ("CinQ = 96 on the BIG kernel: half-empty 64-channel ci tile", "direct", 3, 96, 64, 16, 16, 3, 0, 0, 0),
    ("Cin = 160 / Cout = 320: tile variant 128 x 64", "1x1", 8, 160, 320, 8, 8, 1, 0, 0, 0),
    ("Cin = 320 / Cout = 160: tile variant 64 x 128", "1x1", 8, 320, 160, 8, 8, 1, 0, 0, 0),
    # (the enumeration's representatives are the cheapest, i.e. the narrowest, layers of their classes)
    ("two co x two ci tiles, two tiles a slice, short last slice", "direct", 133, 96, 96, 8, 8, 3, 0, 0, 0),
    ("two co x three ci tiles, stride 2, two tiles a slice, short last slice", "direct", 173, 96, 96, 8, 8, 3, 1, 0, 0),
    ("two co x four ci tiles, three chunks a slice, short last slice, db + db2", "f44", 17, 128, 128, 16, 16, 3, 0, 0, 2),
    # the bench step's three stride-2 layers at S = 96 (64->64 @32: 768 tiles in 256 slices; 128->128 @16: 192 in 64;
    # 192->192 @8: 48 in 24), channels scaled down to the cap with (units, z, per) unchanged (BENCH_PLANS)
    ("bench stride-2 64->64 @32, S = 96", "direct", 96, 64, 16, 32, 32, 3, 1, 0, 0),
    ("bench stride-2 128->128 @16, S = 96", "direct", 96, 192, 16, 16, 16, 3, 1, 0, 0),
    ("bench stride-2 192->192 @8, S = 96", "direct", 96, 352, 32, 8, 8, 3, 1, 0, 0),
)
# (full-size layer, its scaled stand-in above): same (units, z, per, last)
BENCH_PLANS = (((96, 64, 64, 32), (96, 64, 16, 32)), ((96, 128, 128, 16), (96, 192, 16, 16)), ((96, 192, 192, 8), (96, 352, 32, 8)))


def _grid():
    S = np.arange(1, S_MAX + 1, dtype=np.int64)[:, None, None]
    Ci = np.array(CHANNELS, dtype=np.int64)[None, :, None]
    Co = np.array(CHANNELS, dtype=np.int64)[None, None, :]
    return S, Ci, Co


@functools.lru_cache(maxsize=None)
def _order():
    """The domain's points cheapest first: two or more views first (a view stride cannot go wrong on one), then the
    fewest multiply-adds (S Cin Cout: the map and KS are fixed within a sweep), then the smaller S, Cin, Cout."""
    S, Ci, Co = _grid()
    shape = (S.size, Ci.size, Co.size)
    s, ci, co = (np.broadcast_to(a, shape).ravel() for a in (S, Ci, Co))
    order = np.lexsort((co, ci, s, s * ci * co, s < 2))
    return shape, order, s[order], ci[order], co[order]


def _cheapest(keys, valid=None):
    """{key: (S, Cin, Cout)}: per (small non-negative integer) class key its first point in _order()."""
    shape, order, s, ci, co = _order()
    k = np.broadcast_to(keys, shape).ravel()[order]
    idx = np.arange(k.size) if valid is None else np.nonzero(np.broadcast_to(valid, shape).ravel()[order])[0]
    k = k[idx]
    first = np.full(int(k.max()) + 1, -1, dtype=np.int64)
    first[k[::-1]] = idx[::-1]                                # (the last write wins: the smallest index)
    return {key: (int(s[i]), int(ci[i]), int(co[i])) for key, i in enumerate(first) if i >= 0}


@functools.lru_cache(maxsize=None)
def _enumerate():
    found = collections.OrderedDict()      # Case fields without `why` -> [why]
    best = {}                              # a key without a map in it (1x1 halves, reduce) -> (sort key, Case)
    S, Ci, Co = _grid()

    def add(c, why):
        found.setdefault(tuple(c)[:-1], []).append(why)

    def offer(cls, c):
        sk = (c.S < 2, cost(c), c.S, c.Cin, c.Cout, FAMILIES.index(c.family), c.H, c.W, c.mode, c.C1)
        if cls not in best or sk < best[cls][0]:
            best[cls] = (sk, c)

    def sweep(family, H, W, KS, mode, d, key, dbs=(0,)):
        if key is not None:
            for _, (s, ci, co) in sorted(_cheapest(key).items()):
                for db in dbs:
                    c = Case(family, s, ci, co, H, W, KS, mode, 0, db, "")
                    add(c, "class " + " ".join(str(v) for v in plan_class(c)[1:]))
        for _, (s, ci, co) in _cheapest(_nslab_bucket(d["z"]) * 2 + _ragged(d["nt"], Ci, Co)).items():
            c = Case(family, s, ci, co, H, W, KS, mode, 0, dbs[-1], "")
            offer(reduce_class(c), c)

    for mode, maps in sorted(DIRECT_MAPS.items()):
        for W in maps:
            d = plan_direct(S, Ci, Co, W, mode)
            sweep("direct", W, W, 3, mode, d, (_bucket3(d["per"]) * 2 + (d["last"] < d["per"])) * 2 + d["half"])
    for W in ONE_MAPS:
        d = plan_1x1(S, Ci, Co, W)
        tiles = ((d["tm"] // 128) * 2 + d["tn"] // 128) * 4 + (d["CoutP"] > Co) * 2 + (d["CinQ"] > Ci)
        slices = (np.minimum(d["per"], 8) * 2 + (d["last"] < d["per"])) * 2 + (d["z"] == 1)
        for C1 in (0, 64, 128):            # none | inside a 128-wide ci tile, on a 64-wide tile's edge | on a 128-wide tile's edge
            for _, (s, ci, co) in _cheapest(tiles, (d["z"] > 1) & (Ci > C1)).items():       # (two or more slices of >= 4 steps)
                c = Case("1x1", s, ci, co, W, W, 1, 0, C1, 0, "")
                offer(plan_classes(c)[0], c)
        for _, (s, ci, co) in _cheapest(slices).items():
            c = Case("1x1", s, ci, co, W, W, 1, 0, 0, 0, "")
            offer(plan_classes(c)[1], c)
        sweep("1x1", W, W, 1, 0, d, None)
    for W in F44_MAPS:
        for mode in F44_MODES:
            d = plan_f44(S, Ci, Co, W, mode)
            sweep("f44", W, W, 3, mode, d, _bucket3(d["per"]) * 2 + (d["last"] < d["per"]), dbs=(0, 1, 2))
    for H, W, KS, mode in ANY_SHAPES:
        d = plan_any(S, Ci, Co, H, W, KS, mode)
        sweep("any", H, W, KS, mode, d, (_bucket3(d["per"]) * 2 + (d["last"] < d["per"])) * 2 + d["partial_step"])
    for why, *fields in SPECIALS:
        add(Case(*fields, ""), why)
    for cls, (_, c) in sorted(best.items(), key=lambda kv: str(kv[0])):
        if cls[0] != "reduce":
            add(c, "class " + " ".join(str(v) for v in cls))
    have = {reduce_class(Case(*k, "")) for k in found}
    for cls, (_, c) in sorted(best.items(), key=lambda kv: str(kv[0])):
        if cls[0] == "reduce" and cls not in have:
            add(c, "reduce class " + " ".join(str(v) for v in cls[1:]))
            have.add(cls)
    return tuple(Case(*k, "; ".join(dict.fromkeys(v))) for k, v in found.items())


def cases():
    return list(_enumerate())


def covered_classes():
    cs = cases()
    return {k for c in cs for k in plan_classes(c)} | {reduce_class(c) for c in cs}


def hygiene_cases():
    """Per family: the cheapest cases with a short last slice, one slice only, the most slices, and the family's own edge
    (half-empty 8x8 tile, concatenated input, db + db2, partial last step)."""
    out = []
    for fam in FAMILIES:
        cs = sorted((c for c in cases() if c.family == fam), key=lambda c: (cost(c), case_id(c)))
        D = {c: plan(c) for c in cs}
        edge = {"direct": lambda c: D[c]["half"], "1x1": lambda c: c.C1, "f44": lambda c: c.db == 2,
                "any": lambda c: D[c]["partial_step"]}[fam]
        picks = [next(c for c in cs if D[c]["last"] < D[c]["per"] and D[c]["z"] > 1), next(c for c in cs if D[c]["z"] == 1),
                 max(cs, key=lambda c: (D[c]["z"], -cost(c))),
                 min((c for c in cs if edge(c)), key=lambda c: (D[c]["z"] == 1, cost(c), case_id(c)))]
        out += list(dict.fromkeys(picks))
    return out


def clip_cases():
    """Per family the cheapest case whose preferred plan has eight or more slices (F(4x4): with db + db2)."""
    out = []
    for fam in FAMILIES:
        cs = sorted((c for c in cases() if c.family == fam and plan(c)["z"] >= 8 and (fam != "f44" or c.db == 2)),
                    key=lambda c: (cost(c), case_id(c)))
        out.append(cs[0])
    return out


# ------------------------------------------------------------------------------------------------ inputs and references
def rnd(*shape, seed=0):
    """Seeded uniform values in (-1, 1), float32 (the inputs of tests/test_gpu_kernels.py)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def in_size(c):
    return {0: (c.H, c.W), 1: (2 * c.H, 2 * c.W), 2: (c.H // 2, c.W // 2)}[c.mode]


def inputs(c):
    """-> dict(x (the whole input, both parts of a concatenation), gy), float32 on the CPU."""
    Hi, Wi = in_size(c)
    return dict(x=rnd(c.S, c.Cin, Hi, Wi, seed=7), gy=rnd(c.S, c.Cout, c.H, c.W, seed=10))


def tols(c):
    return (TOL_DW, TOL_DB, TOL_DB)[:1 + c.db]


def _seen(x, c):
    """The input as the conv sees it (mode 2: nearest-upsampled)."""
    return F.interpolate(x, scale_factor=2, mode="nearest") if c.mode == 2 else x


def wgrad_ref(t, c, dtype):
    """F.conv2d's weight gradient in `dtype` on the CPU (+ the channel sums of dY for db / db2) -> [dW, (db, (db2))]."""
    w = torch.zeros(c.Cout, c.Cin, c.KS, c.KS, dtype=dtype, requires_grad=True)
    y = F.conv2d(_seen(t["x"].to(dtype), c), w, stride=2 if c.mode == 1 else 1, padding=c.KS // 2)
    y.backward(t["gy"].to(dtype))
    db = t["gy"].to(dtype).sum((0, 2, 3))
    return [w.grad] + [db] * c.db


# ------------------------------------------------------------------------------------------------ the slab model
def unit_pixels(c, d):
    """(units * UNIT_PX,) global output-pixel indices (s H W + y W + x) in the order the launch walks them; -1 where a
    unit reaches past the data (the missing image of a half-empty 8x8 tile, the tail of a partly filled step)."""
    upx, npix = UNIT_PX[c.family], c.S * c.H * c.W
    if c.family == "f44":
        W = c.W
        tpr = min(W // 4, 4)
        tr = 4 // tpr
        cpr = (W // 4) // tpr
        cpi = (W // 4) // tr * cpr
        u = torch.arange(d["units"])
        s, r = u // cpi, u % cpi
        y0, x0 = (r // cpr) * tr * 4, (r % cpr) * tpr * 4
        yy, xx = torch.meshgrid(torch.arange(4 * tr), torch.arange(4 * tpr), indexing="ij")
        idx = (s * W * W)[:, None] + ((y0[:, None] + yy.reshape(1, -1)) * W + x0[:, None] + xx.reshape(1, -1))
        return idx.reshape(-1)
    idx = torch.arange(d["units"] * upx)
    return torch.where(idx < npix, idx, torch.full_like(idx, -1))


MUTANTS = ("drop_last_unit", "shift_ranges", "skip_slab", "reread_last_image", "fold_padding")


def mutant_applies(c, d, m):
    if m == "reread_last_image":
        return d["half"]
    if m == "fold_padding":
        # only the 1x1 and F(4x4) kernels load a padded row as a DUPLICATE of the last channel (the direct and the general
        # kernels load zeros there: folding those in changes nothing, by construction)
        return c.family in ("1x1", "f44") and (d["CoutP"] > c.Cout or d["CinQ"] > c.Cin)
    return True


def _sum8(parts, skip):
    """wgrad_reduce_body / the bias rows of wino44_reduce_body: thread group g of 4 walks slabs g, g + 32, ... with eight
    accumulators at stride 4."""
    n, red = len(parts), []
    for g in range(4):
        a8 = [torch.zeros_like(parts[0]) for _ in range(8)]
        for s in range(g, n, 32):
            for j in range(8):
                if s + 4 * j < n and s + 4 * j != skip:
                    a8[j] = a8[j] + parts[s + 4 * j]
        red.append(((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7])))
    return (red[0] + red[1]) + (red[2] + red[3])


def _sum2(parts, skip):
    """wino44_reduce_body: thread group g walks slabs g, g + 4, ... with two accumulators (g + 8 k | g + 4 + 8 k)."""
    n, red = len(parts), []
    zero = torch.zeros_like(parts[0])
    get = lambda k: zero if k == skip else parts[k]
    for g in range(4):
        c0, c1 = zero.clone(), zero.clone()
        z = g
        while z + 4 < n:
            c0, c1 = c0 + get(z), c1 + get(z + 4)
            z += 8
        if z < n:
            c0 = c0 + get(z)
        red.append(c0 + c1)
    return (red[0] + red[1]) + (red[2] + red[3])


def reduce_trips(nslab):
    """Per thread group the slabs of each trip of wgrad_reduce_body's loop (the masked loads left out)."""
    return [[[s + 4 * j for j in range(8) if s + 4 * j < nslab] for s in range(g, nslab, 32)] for g in range(4)]


def wgrad_slabs(t, c, d, mutate=None, dtype=torch.float32, cache=None):
    """The slab decomposition on the CPU: one partial dW (and dY sum) per slice over exactly that slice's units, then
    the slab sum's grouping and order -> [dW, (db, (db2))].  mutate: one of MUTANTS.  cache: a dict that lives as long
    as (t, c, d, dtype) do; it keeps the unfolded input and the partials that several mutants share."""
    assert mutate is None or (mutate in MUTANTS and mutant_applies(c, d, mutate))
    cache = {} if cache is None else cache
    npix = c.S * c.H * c.W
    if "xu" not in cache:
        x, gy = _seen(t["x"].to(dtype), c), t["gy"].to(dtype)
        xu = F.unfold(x, c.KS, padding=c.KS // 2, stride=2 if c.mode == 1 else 1)              # (S, Cin KS^2, H W)
        cache["xu"] = xu.permute(1, 0, 2).reshape(c.Cin * c.KS * c.KS, npix)
        cache["g2"] = gy.permute(1, 0, 2, 3).reshape(c.Cout, npix)
    xu, g2 = cache["xu"], cache["g2"]
    upx, units, per, z = UNIT_PX[c.family], d["units"], d["per"], d["z"]
    walk = mutate if mutate in ("reread_last_image", "drop_last_unit", "shift_ranges") else None
    if ("parts", walk) not in cache:
        order = unit_pixels(c, d)
        if walk == "reread_last_image":
            hw = c.H * c.W
            order[-hw:] = torch.arange((c.S - 1) * hw, c.S * hw)
        if walk == "drop_last_unit":
            order[(units - 1) * upx:] = -1
        shift = 1 if walk == "shift_ranges" else 0
        parts, bparts = [], []
        for i in range(z):
            idx = order[(i * per + shift) * upx:min(units, (i + 1) * per + shift) * upx]
            idx = idx[idx >= 0]
            parts.append((g2[:, idx] @ xu[:, idx].T).reshape(c.Cout, c.Cin, c.KS, c.KS))
            bparts.append(g2[:, idx].sum(1))
        cache["parts", walk] = (parts, bparts)
    parts, bparts = cache["parts", walk]
    skip = min(32, z - 1) if mutate == "skip_slab" else None
    dw = (_sum2 if d["nt"] == 0 else _sum8)(parts, skip)
    db = _sum8(bparts, skip)
    if mutate == "fold_padding":
        dw, db = dw.clone(), db.clone()
        dw[0] += (d["CoutP"] - c.Cout) * dw[c.Cout - 1]
        dw[:, 0] += (d["CinQ"] - c.Cin) * dw[:, c.Cin - 1]
        db[0] += (d["CoutP"] - c.Cout) * db[c.Cout - 1]
    return [dw] + [db] * c.db
