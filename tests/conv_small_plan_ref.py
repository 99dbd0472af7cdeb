"""The launch plan of the sampler's one-launch convolutions restated in pure Python -- conv_small_plan
(csrc/conv_small.hip: every refusal branch in the launcher's order, conv1_small_kernel<CAT> / conv3_small_kernel<LOGTC, RS,
PACKED>, grid, the per-wave shares n / rn, rounds and the last round's channels), vf_conv_small_supported,
vf_conv_small_pack_floats and the policy of ops (use_small_conv, can_fold_residual) -- with the index algebra of the kernels
as numpy, the plan-class enumeration behind tests/test_gpu_conv_small_plan.py, the inputs, the float64 / stock fp32
references and the seven wrong models those tests share.

A coverage key (class_keys) is one decision of the launcher or one path of a kernel, crossed with what the code around it
distinguishes:
  ("inst", kernel, LOGTC, RS, PACKED)                  the fourteen instantiations
  ("rounds", nr class, last round, RS, PACKED)         3x3: nr in {1, 2, >= 3} x a full (8-channel) / half (4) last round
  ("share", "1x1" | "cat" | "fold", class)             the per-wave share of a 1x1 K loop: "whole" (every wave full),
                                                       "partial" (a partly filled wave), "empty" (wholly empty waves),
                                                       "clamp" (K = 4: the K - 4 clamp is 0), "second trip" (K > 512)
  ("cout", kind, RS, PACKED, class)                    Cout % (16 RS): "0", "1..16", "17..31" (the last needs RS = 2)
  ("boundary", "cat" | "fold", "on 4" | "off 4")       the concatenation boundary against the groups of four channels
  ("epi", kind, operand, present)                      bias, vbias, residual; ("rbias", present) for the folded conv
  ("fold", RS, PACKED)                                 the folded residual conv behind each form of the 3x3 main loop
  ("gn", kind, cpg class, silu)                        GroupNorm on load: cpg "1", "several", "straddle" (a group whose
                                                       channels lie in two waves); ("gn limit", kind): 1x1 Cin = 1024,
                                                       3x3 Cin / 8 = 64
  ("ostats", kind, RS, on) and ("ostats partial", kind, RS)   output statistics; on a partial channel tile
  ("up", LOGTC, RS, PACKED)                            the Upsample conv
cases() holds, for every key of required_keys(), the cheapest case -- by cost() = S Cout (KS^2 Cin + rC) H W -- of a
generated candidate domain that has the key.  Imports no GPU code."""
import collections
import functools
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

import cond_ref as cr

MAX_COST = 2e8                                          # multiply-adds per case
SEED = 71
GN_MAXC, GN_MAXCW = 1024, 64                            # SM_GN_MAXC; most channels per wave with GroupNorm on load (3x3)
INVALID = 1                                             # hipErrorInvalidValue

# vf_conv_small_plan's arguments and out[16]
ARGS = ("S", "Cin", "Cout", "H", "W", "KS", "mode", "x2", "C1", "ist", "affine", "groups", "ost", "rx", "rx2", "rC1", "rC",
        "rw", "residual", "wp")
FIELDS = ("code", "kernel", "logtc", "rs", "packed", "grid", "n", "rn", "nr", "last", "up", "gn", "ostats", "fold", "logW",
          "icpg")
K_NONE, K_1X1, K_CAT, K_3X3 = 0, 1, 2, 3
KIND = {K_1X1: "1x1", K_CAT: "cat", K_3X3: "3x3"}
REFUSALS = {1: "unsupported layer", 2: "x2 on a 3x3 conv or C1 outside (0, Cin)", 3: "in_stats with x2",
            4: "in_stats without gamma / beta", 5: "in_groups <= 0", 6: "Cin % in_groups != 0", 7: "1x1 in_stats, Cin > 1024",
            8: "3x3 in_stats, Cin / 8 > 64", 9: "mode 2 with rx or in_stats", 10: "rx on a 1x1 conv", 11: "rx with a residual",
            12: "rx without rw", 13: "rC < 4", 14: "rC % 4 != 0", 15: "rC1 outside (0, rC)"}
# natural thresholds of ops.state: (1x1 workgroups, 3x3 workgroups), 3x3 Cin, 3x3 views
NATURAL = dict(wgs1=1024, wgs3=512, cin3=256, s3=1)
OPEN = dict(wgs1=1 << 30, wgs3=1 << 30, cin3=1 << 30, s3=1 << 30)


def _roundup16(v):
    return (v + 15) & ~15


# ------------------------------------------------------------------------------------------------ the planner
def supported(Cin, Cout, H, W, KS, mode):
    """vf_conv_small_supported; ints or int64 arrays."""
    Cin, Cout, H, W, KS, mode = (np.asarray(v, dtype=np.int64) for v in (Cin, Cout, H, W, KS, mode))
    geom = (H == W) & (H >= 4) & ((H & (H - 1)) == 0) & (Cin >= 1) & (Cout >= 1)
    mode_ok = (mode == 0) | ((mode == 2) & (KS == 3) & (H >= 8))
    return (geom & mode_ok & (((KS == 1) & (Cin % 4 == 0)) | ((KS == 3) & (Cin % 32 == 0)))).astype(np.int64)


def pack_floats(Cout, Cin):
    """vf_conv_small_pack_floats."""
    Cout, Cin = np.asarray(Cout, dtype=np.int64), np.asarray(Cin, dtype=np.int64)
    cw = Cin >> 3
    return ((Cout + 31) // 32) * 2 * 8 * ((cw + 7) // 8) * 5 * 64 * 4


def plan_arrays(**kw):
    """conv_small_plan -> dict of FIELDS; every ARGS value an int or an int64 array (broadcast together).  rC1 / rC as
    passed to vf_conv_small_gn (the entry's normalisation -- rC1 = rC without rx2, both 0 without rx -- is restated here)."""
    a = dict(zip(ARGS, np.broadcast_arrays(*(np.asarray(kw[k], dtype=np.int64) for k in ARGS))))
    S, Cin, Cout, H, W, KS, mode, C1, groups = (a[k] for k in ("S", "Cin", "Cout", "H", "W", "KS", "mode", "C1", "groups"))
    x2, ist, affine, ost, rx, rx2, rw, residual, wp = (a[k] != 0 for k in ("x2", "ist", "affine", "ost", "rx", "rx2", "rw",
                                                                           "residual", "wp"))
    rC = np.where(rx, a["rC"], 0)
    rC1 = np.where(rx, np.where(rx2, a["rC1"], rC), 0)
    gsafe = np.where(groups > 0, groups, 1)
    tests = [(supported(Cin, Cout, H, W, KS, mode) == 0, 1),
             (x2 & ((KS != 1) | (C1 <= 0) | (C1 >= Cin)), 2),
             (ist & x2, 3), (ist & ~affine, 4), (ist & (groups <= 0), 5), (ist & (Cin % gsafe != 0), 6),
             (ist & (KS == 1) & (Cin > GN_MAXC), 7), (ist & (KS == 3) & (Cin // 8 > GN_MAXCW), 8),
             ((mode == 2) & (rx | ist), 9),
             (rx & (KS != 3), 10), (rx & residual, 11), (rx & ~rw, 12), (rx & (rC < 4), 13), (rx & (rC % 4 != 0), 14),
             (rx & np.where(rx2, (rC1 <= 0) | (rC1 >= rC), rC1 != rC), 15)]
    code = np.zeros_like(S)
    for cond, c in reversed(tests):                      # the first test that fires wins
        code = np.where(cond, c, code)
    run = (code == 0) & (S > 0)
    is3 = KS == 3
    Ws = np.where(W > 0, W, 1)
    logW = np.ceil(np.log2(Ws)).astype(np.int64)
    wgs32 = S * ((Cout + 31) // 32) * (H * W // 16)
    kernel = np.where(is3, K_3X3, np.where(x2, K_CAT, K_1X1))
    rs = np.where(is3, np.where(wgs32 >= 256, 2, 1), 2)
    cw = Cin >> 3
    nr = (cw + 7) // 8
    z = lambda v: np.where(run, v, 0)
    z3 = lambda v: np.where(run & is3, v, 0)
    return dict(code=code, kernel=z(kernel), logtc=z3(np.where(W >= 16, 4, np.where(W == 8, 3, 2))), rs=z(rs),
                packed=z3(wp.astype(np.int64)), grid=z(S * ((Cout + 16 * rs - 1) // (16 * rs)) * (H * W // 16)),
                n=z(_roundup16((Cin + 7) // 8)), rn=z(np.where(rx, _roundup16((rC + 7) // 8), 0)), nr=z3(nr),
                last=z3(cw - (nr - 1) * 8), up=z((mode == 2).astype(np.int64)), gn=z(ist.astype(np.int64)),
                ostats=z(ost.astype(np.int64)), fold=z(rx.astype(np.int64)), logW=z(logW),
                icpg=z(np.where(ist, Cin // gsafe, 1)))


def fields(d):
    return [int(d[k]) for k in FIELDS]


# ------------------------------------------------------------------------------------------------ the policy of ops
def use_small(S, Cin, Cout, H, W, KS, m, thr=NATURAL):
    """ops.use_small_conv (SMALL_CONV on)."""
    if not int(supported(Cin, Cout, H, W, KS, m)):
        return False
    wgs = S * ((Cout + 31) // 32) * (H * W // 16)
    if KS == 1:
        return wgs <= thr["wgs1"]
    return wgs <= thr["wgs3"] and Cin <= thr["cin3"] and S <= thr["s3"]


def can_fold(S, C, H, W, rC, thr=NATURAL):
    """ops.can_fold_residual for a 1x1 residual conv of rC input channels (RES_FOLD on, autograd off); rC None: Identity."""
    return rC is not None and rC % 4 == 0 and use_small(S, C, C, H, W, 3, 0, thr)


# ------------------------------------------------------------------------------------------------ index algebra as numpy
def conv3_map(Cin):
    """The slots of conv3_small_kernel: -> dict of flat int arrays over (wave 8, round nr, group q 5, quarter kk 4, e 4):
    valid (the weight is kept), wch / wtap (channel and tap of the OIHW float the unpacked load reads: wa + r 72 + 16 q + e,
    wa = c0 9 + 4 kk), bch / btap (channel and tap the B table addresses), rereads (the group past the round's products
    that re-reads group 0), off (row offset of the float the unpacked load really reads)."""
    cw = Cin >> 3
    nr = (cw + 7) // 8
    w, r, q, kk, e = (v.ravel() for v in np.meshgrid(np.arange(8), np.arange(nr), np.arange(5), np.arange(4), np.arange(4),
                                                      indexing="ij"))
    np_ = 9 * np.minimum(8, cw - 8 * r)
    k = 16 * q + 4 * kk + e
    valid = 16 * q + 4 * kk < np_
    c0 = w * cw
    off = c0 * 9 + 4 * kk + r * 72 + np.where(valid, 16 * q, 0) + e
    kc = np.minimum(k, 71)
    ci = (kc * 57) >> 9
    tap = kc - 9 * ci
    dy = (tap * 11) >> 5
    return dict(valid=valid, wch=c0 + 8 * r + k // 9, wtap=k % 9, bch=c0 + 8 * r + ci, btap=3 * dy + (tap - 3 * dy), off=off,
                k=k, np=np_, wave=w, round=r, q=q, kk=kk, e=e, dy=dy, dx=tap - 3 * dy)


def conv1_map(K, n=None):
    """The slots of conv1_small_kernel's (and the fold's) K loop: -> dict over (wave 8, trip, q 4, kk 4, e 4): ok, k (the
    channel the slot stands for), load (the channel really loaded: min(k, K - 4) + e)."""
    n = int(_roundup16((K + 7) // 8)) if n is None else n
    trips = (n + 63) // 64
    w, t, q, kk, e = (v.ravel() for v in np.meshgrid(np.arange(8), np.arange(trips), np.arange(4), np.arange(4), np.arange(4),
                                                      indexing="ij"))
    mb = 64 * t
    k = w * n + 4 * kk + mb + 16 * q
    ok = (mb + 16 * q < n) & (k < K)
    return dict(ok=ok, k=k + e, load=np.minimum(k, K - 4) + e, wave=w, n=n, trips=trips, issued=mb + 16 * q < n)


def pack_numpy(w):
    """conv3_small_pack_kernel on an OIHW array (Cout, Cin, 3, 3) -> the packed floats, and the flat OIHW index of every
    packed float (-1 where the kernel writes a zero)."""
    Cout, Cin = w.shape[:2]
    cw = Cin >> 3
    nr = (cw + 7) // 8
    n4 = int(pack_floats(Cout, Cin)) // 4
    idx = np.arange(n4)
    lane, q, r = idx & 63, (idx >> 6) % 5, (idx // 320) % nr
    wv, blk = (idx // (320 * nr)) & 7, idx // (320 * nr * 8)
    j, kk = lane & 15, lane >> 4
    co = blk * 16 + j
    np_ = 9 * np.minimum(8, cw - r * 8)
    k0 = 16 * q + 4 * kk
    keep = (co < Cout) & (k0 < np_)
    src = (co * Cin * 9 + (wv * cw + r * 8) * 9 + k0)[:, None] + np.arange(4)[None, :]
    src = np.where(keep[:, None], src, -1)
    flat = np.concatenate([w.reshape(-1), np.zeros(1, w.dtype)])
    return flat[src].reshape(-1), src.reshape(-1)


def packed_read_index(Cout, Cin, RS, cot, rs, wave, R, q, lane):
    """float4 index conv3_small_kernel<., RS, true> reads: wpk[rs][((R) NQ + q) 64]."""
    nrp = ((Cin >> 3) + 7) // 8
    return ((cot * RS + rs) * 8 + wave) * nrp * 320 + lane + (R * 5 + q) * 64


def tile_geometry(W, up=False):
    """conv3_small_kernel's tile and patch coordinates on a W x W output map -> dict:
    pix[pt][j] = flat output pixel of lane j of tile pt; src[pt][l] = flat index into the stored x plane of patch element l
    (-1: zero padding, or a lane past the patch); tap[j][dy][dx] = patch element that pixel j's tap (dy, dx) reads."""
    logtc = 4 if W >= 16 else (3 if W == 8 else 2)
    logW = int(math.log2(W))
    TC = 1 << logtc
    TR, PC = 16 // TC, TC + 2
    PS = (TR + 2) * PC
    pt = np.arange(W * W // 16)
    p0 = pt * 16
    ty0, tx0 = p0 >> logW, p0 & (W - 1)
    j = np.arange(16)
    pix = (ty0[:, None] + (j >> logtc)[None, :]) * W + tx0[:, None] + (j & (TC - 1))[None, :]
    lane = np.arange(64)
    pr = lane // PC
    pc = lane - pr * PC
    gy, gx = ty0[:, None] + pr[None, :] - 1, tx0[:, None] + pc[None, :] - 1
    pin = (lane[None, :] < PS) & (gy >= 0) & (gy < W) & (gx >= 0) & (gx < W)
    src = np.where(pin, (gy >> 1) * (W >> 1) + (gx >> 1) if up else gy * W + gx, -1)
    tap = ((j >> logtc) * PC + (j & (TC - 1)))[:, None, None] + (np.arange(3) * PC)[None, :, None] + np.arange(3)[None, None, :]
    return dict(logtc=logtc, PS=PS, PC=PC, pix=pix, src=src, tap=tap)


# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "S Cin Cout H KS mode C1 bias vbias residual rC rC1 rbias groups silu ostats packed why")


def mk(S, Cin, Cout, H, KS=3, mode=0, C1=0, bias=1, vbias=0, residual=0, rC=0, rC1=0, rbias=0, groups=0, silu=0, ostats=0,
       packed=0, why=""):
    """rC > 0: the folded residual conv, rC1 > 0: split [rx | rx2] at rC1; groups > 0: GroupNorm on load; C1 > 0: x2."""
    return Case(*(int(v) for v in (S, Cin, Cout, H, KS, mode, C1, bias, vbias, residual, rC, rC1, rbias, groups, silu, ostats,
                                   packed)), why)


def case_id(c):
    s = f"S{c.S}-{c.Cin}to{c.Cout}-{c.H}x{c.H}-k{c.KS}" + ("-up" if c.mode == 2 else "") + (f"-cat{c.C1}" if c.C1 else "")
    s += "-" + "".join(ch for ch, on in zip("bvr", (c.bias, c.vbias, c.residual)) if on) if (c.bias or c.vbias or c.residual) else ""
    if c.rC:
        s += f"-fold{c.rC}" + (f"at{c.rC1}" if c.rC1 else "") + ("rb" if c.rbias else "")
    if c.groups:
        s += f"-gn{c.groups}" + ("silu" if c.silu else "")
    return s + ("-stats" if c.ostats else "") + ("-packed" if c.packed else "")


def cost(c):
    return c.S * c.Cout * (c.KS * c.KS * c.Cin + c.rC) * c.H * c.H


def entry(c):
    """The C-ABI entry a case runs through: the narrowest one that takes its operands."""
    if c.groups or c.ostats or c.packed or (c.rC and c.residual):
        return "vf_conv_small_gn"
    return "vf_conv_small_res" if c.rC else "vf_conv_small"


def plan_args(c, **over):
    a = dict(S=c.S, Cin=c.Cin, Cout=c.Cout, H=c.H, W=c.H, KS=c.KS, mode=c.mode, x2=int(c.C1 > 0), C1=c.C1,
             ist=int(c.groups > 0), affine=int(c.groups > 0), groups=c.groups, ost=c.ostats, rx=int(c.rC > 0),
             rx2=int(c.rC1 > 0), rC1=c.rC1, rC=c.rC, rw=int(c.rC > 0), residual=c.residual, wp=c.packed)
    a.update(over)
    return a


def plan(c, **over):
    return {k: int(v) for k, v in plan_arrays(**plan_args(c, **over)).items()}


def _share_classes(K):
    n = int(_roundup16((K + 7) // 8))
    out = []
    filled = [min(max(K - w * n, 0), n) for w in range(8)]
    if all(f == n for f in filled):
        out.append("whole")
    if any(0 < f < n for f in filled):
        out.append("partial")
    if any(f == 0 for f in filled):
        out.append("empty")
    if K == 4:
        out.append("clamp")
    if n > 64:
        out.append("second trip")
    return out


def _straddles(c, d):
    cpg = c.Cin // c.groups
    per_wave = c.Cin >> 3 if c.KS == 3 else d["n"]
    return any((g * cpg) // per_wave != (g * cpg + cpg - 1) // per_wave for g in range(c.groups))


def class_keys(c):
    """The coverage keys of case c ([] for a refused case)."""
    d = plan(c)
    if d["code"] or d["kernel"] == K_NONE:
        return []
    kind = KIND[d["kernel"]]
    rs, pk = d["rs"], d["packed"]
    keys = [("inst", kind, d["logtc"], rs, pk)]
    if kind == "3x3":
        keys.append(("rounds", "1" if d["nr"] == 1 else "2" if d["nr"] == 2 else ">= 3", d["last"], rs, pk))
        if c.mode == 2:
            keys.append(("up", d["logtc"], rs, pk))
    else:
        keys += [("share", kind, k) for k in _share_classes(c.Cin)]
    if c.rC:
        keys += [("share", "fold", k) for k in _share_classes(c.rC)]
        keys += [("rbias", c.rbias), ("fold", rs, pk)]
        if c.rC1:
            keys.append(("boundary", "fold", "on 4" if c.rC1 % 4 == 0 else "off 4"))
    if c.C1:
        keys.append(("boundary", "cat", "on 4" if c.C1 % 4 == 0 else "off 4"))
    m = c.Cout % (16 * rs)
    keys.append(("cout", kind, rs, pk, "0" if m == 0 else "1..16" if m <= 16 else "17..31"))
    keys += [("epi", kind, n, int(on)) for n, on in (("bias", c.bias), ("vbias", c.vbias), ("residual", c.residual))]
    if c.groups:
        cpg = c.Cin // c.groups
        keys.append(("gn", kind, "1" if cpg == 1 else "straddle" if _straddles(c, d) else "several", c.silu))
        if (c.KS == 1 and c.Cin == GN_MAXC) or (c.KS == 3 and c.Cin // 8 == GN_MAXCW):
            keys.append(("gn limit", kind))
    keys.append(("ostats", kind, rs, c.ostats))
    if c.ostats and m:
        keys.append(("ostats partial", kind, rs))
    return keys


def required_keys():
    """The keys the kernels' code distinguishes, from arithmetic alone."""
    req = {("inst", "1x1", 0, 2, 0), ("inst", "cat", 0, 2, 0)}
    for rs, pk in itertools.product((1, 2), (0, 1)):
        req |= {("inst", "3x3", ltc, rs, pk) for ltc in (4, 3, 2)} | {("up", ltc, rs, pk) for ltc in (4, 3)}
        req |= {("rounds", nr, last, rs, pk) for nr in ("1", "2", ">= 3") for last in (8, 4)}
        req |= {("cout", "3x3", rs, pk, m) for m in (("0", "1..16", "17..31") if rs == 2 else ("0", "1..16"))}
    for kind in ("1x1", "cat"):
        req |= {("cout", kind, 2, 0, m) for m in ("0", "1..16", "17..31")}
    req |= {("share", "1x1", k) for k in ("whole", "partial", "empty", "clamp", "second trip")}
    req |= {("share", "cat", k) for k in ("whole", "partial", "empty", "clamp", "second trip")}
    req |= {("share", "fold", k) for k in ("whole", "partial", "empty", "clamp", "second trip")}
    req |= {("fold", rs, pk) for rs in (1, 2) for pk in (0, 1)}
    req |= {("boundary", k, b) for k in ("cat", "fold") for b in ("on 4", "off 4")} | {("rbias", 0), ("rbias", 1)}
    req |= {("epi", k, n, on) for k in ("1x1", "cat", "3x3") for n in ("bias", "vbias", "residual") for on in (0, 1)}
    req |= {("gn", k, cls, silu) for k in ("1x1", "3x3") for cls in ("1", "several", "straddle") for silu in (0, 1)}
    req |= {("gn limit", "1x1"), ("gn limit", "3x3")}
    req |= {("ostats", "1x1", 2, on) for on in (0, 1)} | {("ostats", "cat", 2, on) for on in (0, 1)}
    req |= {("ostats", "3x3", rs, on) for rs in (1, 2) for on in (0, 1)}
    req |= {("ostats partial", "1x1", 2), ("ostats partial", "3x3", 1), ("ostats partial", "3x3", 2)}
    return req


# S that reaches the RS = 2 threshold (S ceil(Cout / 32) H W / 16 >= 256) at the Cout below (Cout % 32 = 0, <= 16, > 16),
# per map: the fewest output channels that do it with S <= 64
_RS2 = {4: (64, (128, 100, 120)), 8: (64, (32, 5, 20)), 16: (16, (32, 5, 20))}


def _candidates():
    out = []
    add = lambda *a, **k: out.append(mk(*a, **k))
    # 3x3: rounds x map x RS x PACKED x Cout % tile, plain and Upsample
    for pk in (0, 1):
        for Cin in (32, 64, 96, 128, 160, 192):
            for H in (4, 8, 16):
                for Cout in (5, 16, 20, 32):
                    add(2, Cin, Cout, H, packed=pk)          # (two views: a view / channel index mix-up cannot pass)
                    if H >= 8:
                        add(2, Cin, Cout, H, mode=2, packed=pk)
                S2, couts = _RS2[H]
                for Cout in couts:
                    add(S2, Cin, Cout, H, packed=pk)
                    if H >= 8:
                        add(S2, Cin, Cout, H, mode=2, packed=pk)
    # 1x1 plain / cat: the shares, Cout % 32, the boundary
    for Cin in (4, 8, 12, 64, 68, 128, 132, 516, 1024):
        for Cout in (5, 20, 32):
            add(2, Cin, Cout, 4, KS=1)
            for C1 in (4, 5, Cin - 3):
                if 0 < C1 < Cin:
                    add(2, Cin, Cout, 4, KS=1, C1=C1)
    # epilogue operands, one at a time and none
    for KS, Cin, C1 in ((1, 8, 0), (1, 8, 3), (3, 32, 0)):
        for b, v, r in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            add(2, Cin, 5, 4, KS=KS, C1=C1, bias=b, vbias=v, residual=r)
    # the folded residual conv: shares, boundary, rbias
    for rC in (4, 8, 12, 64, 68, 128, 516):
        for rC1 in (0, 4, 5, rC - 3):
            if 0 <= rC1 < rC:
                for rb in (0, 1):
                    add(2, 32, 5, 4, rC=rC, rC1=rC1, rbias=rb, vbias=1)
    for pk in (0, 1):
        add(2, 32, 5, 4, rC=8, rC1=3, rbias=1, packed=pk)
        add(64, 32, 100, 4, rC=8, rC1=3, rbias=1, packed=pk)
        add(16, 32, 5, 16, rC=8, rC1=3, rbias=1, packed=pk)
    # GroupNorm on load
    for silu in (0, 1):
        for Cin, g in ((32, 32), (32, 8), (96, 12), (96, 4), (512, 32)):
            add(2, Cin, 5, 4, groups=g, silu=silu)
            add(2, Cin, 5, 4, groups=g, silu=silu, packed=1)
        for Cin, g in ((8, 8), (8, 2), (96, 4), (1024, 32)):
            add(2, Cin, 5, 4, KS=1, groups=g, silu=silu)
    # output statistics
    for Cout in (16, 20, 32):
        add(2, 8, Cout, 4, KS=1, ostats=1)
        add(2, 8, Cout, 4, KS=1, C1=3, ostats=1)
        add(2, 32, Cout, 4, ostats=1)
    for H in (4, 8, 16):
        S2, couts = _RS2[H]
        for Cout in couts:
            add(S2, 32, Cout, H, ostats=1)
    return out


@functools.lru_cache(maxsize=None)
def _enumerate():
    best = {}
    for c in _candidates():
        if cost(c) > MAX_COST:
            continue
        for k in class_keys(c):
            cur = best.get(k)
            if cur is None or (cost(c), case_id(c)) < (cost(cur), case_id(cur)):
                best[k] = c
    picked = collections.OrderedDict()
    for k in sorted(best, key=repr):
        picked.setdefault(best[k][:-1], []).append(repr(k))
    return tuple(Case(*k, "; ".join(v)) for k, v in sorted(picked.items(), key=lambda kv: (cost(Case(*kv[0], "")), kv[0])))


def cases():
    return list(_enumerate())


def case_classes():
    return {k for c in cases() for k in class_keys(c)}


def over_cap_classes():
    """Required keys with no representative under MAX_COST."""
    return sorted(required_keys() - case_classes(), key=repr)


def pairs_3x3():
    return [c for c in cases() if c.KS == 3]


def fold_cases():
    return [c for c in cases() if c.rC]


# every refusal branch: (code, case, overrides of plan_args) -- run through vf_conv_small_gn
_B3, _B1 = mk(2, 32, 5, 4), mk(2, 8, 5, 4, KS=1)
REJECTIONS = (
    (1, mk(2, 32, 5, 6), {}), (1, mk(2, 32, 5, 2), {}), (1, mk(2, 16, 5, 4), {}), (1, mk(2, 6, 5, 4, KS=1), {}),
    (1, mk(2, 32, 5, 4, KS=5), {}), (1, mk(2, 32, 5, 4, mode=1), {}), (1, mk(2, 32, 5, 4, mode=2), {}),
    (1, mk(2, 8, 5, 8, KS=1, mode=2), {}), (1, mk(2, 32, 0, 4), {}),
    (2, _B3, dict(x2=1, C1=8)), (2, _B1, dict(x2=1, C1=0)), (2, _B1, dict(x2=1, C1=8)),
    (3, mk(2, 8, 5, 4, KS=1, C1=3, groups=2), {}), (4, mk(2, 32, 5, 4, groups=8), dict(affine=0)),
    (5, _B3, dict(ist=1, affine=1, groups=0)), (5, _B3, dict(ist=1, affine=1, groups=-4)), (6, mk(2, 32, 5, 4, groups=5), {}),
    (7, mk(1, 1028, 5, 4, KS=1, groups=4), {}), (8, mk(1, 544, 5, 4, groups=32), {}),
    (9, mk(2, 32, 5, 8, mode=2, groups=8), {}), (9, mk(2, 32, 5, 8, mode=2, rC=8), {}),
    (10, mk(2, 8, 5, 4, KS=1, rC=8), {}), (11, mk(2, 32, 5, 4, rC=8, residual=1), {}), (12, mk(2, 32, 5, 4, rC=8), dict(rw=0)),
    (13, mk(2, 32, 5, 4, rC=0), dict(rx=1, rw=1)), (14, mk(2, 32, 5, 4, rC=6), {}),
    (15, mk(2, 32, 5, 4, rC=8, rC1=8), {}), (15, mk(2, 32, 5, 4, rC=8), dict(rx2=1, rC1=0)),
)


# ------------------------------------------------------------------------------------------------ the models' layers
def model_layers():
    """Every convolution call of the no-grad forward of the SMALL and TINY networks (view_fusion_amd/unet.py) as
    dict(Cin, Cout, H, KS, mode, C1, bias, vbias, residual, rC, rC1): block convs (the second one with its residual, or
    with the residual conv folded in -- both forms, the policy chooses), residual convs plain and on [x | skip],
    attention projections, Upsample convs, first and final conv."""
    from conftest import SMALL, TINY
    from view_fusion_amd import UNet
    from view_fusion_amd.unet import _ResAttnBlock, _Resample
    out = []

    def add(Cin, Cout, H, KS, mode=0, C1=0, bias=1, vbias=0, residual=0, rC=0, rC1=0):
        L = dict(Cin=Cin, Cout=Cout, H=H, KS=KS, mode=mode, C1=C1, bias=bias, vbias=vbias, residual=residual, rC=rC, rC1=rC1)
        if L not in out:
            out.append(L)

    for hp in (SMALL, TINY):
        net = UNet(**hp)

        def block(blk, H, C1):
            rb = blk.res_block
            c1, c2 = rb.block1["block"]["3"], rb.block2["block"]["3"]
            Cin, Cout = c1.in_channels, c1.out_channels
            add(Cin, Cout, H, 3, vbias=1)
            add(Cout, Cout, H, 3, residual=1)
            if Cin != Cout:
                add(Cin, Cout, H, 1)
                add(Cout, Cout, H, 3, rC=Cin, residual=0)
                if C1:
                    add(Cin, Cout, H, 1, C1=C1)
                    add(Cout, Cout, H, 3, rC=Cin, rC1=C1)
            if blk.with_attn:
                add(Cout, 3 * Cout, H, 1, bias=0)
                add(Cout, Cout, H, 1, residual=1)
            return Cout

        size = lambda conv: hp["image_size"] >> conv._vf_geom[0]
        first = net.downs[0]
        add(first.in_channels, first.out_channels, hp["image_size"], 3)
        ch = first.out_channels
        for layer in list(net.downs)[1:] + list(net.mid):
            if isinstance(layer, _ResAttnBlock):
                ch = block(layer, size(layer.res_block.block1["block"]["3"]), 0)
            elif isinstance(layer, _Resample):
                add(ch, ch, size(layer.conv), 3, mode=1)
        for layer in net.ups:
            if isinstance(layer, _ResAttnBlock):
                ch = block(layer, size(layer.res_block.block1["block"]["3"]), ch)
            else:
                add(ch, ch, size(layer.conv), 3, mode=2)
        fc = net.final_conv["block"]["3"]
        add(fc.in_channels, fc.out_channels, hp["image_size"], 3)
    return out


def layer_case(L, S, packed):
    return mk(S, L["Cin"], L["Cout"], L["H"], KS=L["KS"], mode=L["mode"], C1=L["C1"], bias=L["bias"], vbias=L["vbias"],
              residual=L["residual"], rC=L["rC"], rC1=L["rC1"], rbias=int(L["rC"] > 0), packed=int(packed and L["KS"] == 3))


def reached_classes(thr, S_range=range(1, 25)):
    """-> {key: (layer, S) that first reaches it} over the SMALL / TINY layers under the thresholds thr, packed and not."""
    out = {}
    for L in model_layers():
        for S in S_range:
            if L["rC"]:
                ok = can_fold(S, L["Cout"], L["H"], L["H"], L["rC"], thr)
            else:
                ok = use_small(S, L["Cin"], L["Cout"], L["H"], L["H"], L["KS"], L["mode"], thr)
            if not ok:
                continue
            for packed in (1, 0):
                for k in class_keys(layer_case(L, S, packed)):
                    out.setdefault(k, (tuple(L.values()), S))
    return out


# ------------------------------------------------------------------------------------------------ inputs and references
MUTANTS = ("drop_half_round", "wave_shift", "keep_72_79", "pad_before_gn", "up_in_source", "boundary_off", "no_rbias")


def inputs(c):
    """-> dict of float32 CPU tensors, seeded: x (whole, stored size), w, bias, vbias, residual, rx (whole), rw, rbias,
    gamma, beta; absent operands are None.  With GroupNorm on load x carries a per-(view, group) offset of +-3 sigma."""
    Hs = c.H // 2 if c.mode == 2 else c.H
    u = lambda shape, k: cr._u(shape, SEED + k)
    if c.groups:
        x = cr.gn_input(c.S, c.Cin, Hs, Hs, 3, 1.0, SEED, groups=c.groups)
    else:
        x = u((c.S, c.Cin, Hs, Hs), 0).float()
    t = dict(x=x, w=(u((c.Cout, c.Cin, c.KS, c.KS), 1) / math.sqrt(c.Cin * c.KS * c.KS)).float(),
             bias=(0.1 * u((c.Cout,), 2)).float() if c.bias else None,
             vbias=(0.3 * u((c.S, c.Cout), 3)).float() if c.vbias else None,
             residual=u((c.S, c.Cout, c.H, c.H), 4).float() if c.residual else None,
             rx=None, rw=None, rbias=None, gamma=None, beta=None)
    if c.rC:
        t.update(rx=u((c.S, c.rC, c.H, c.H), 5).float(), rw=(u((c.Cout, c.rC, 1, 1), 6) / math.sqrt(c.rC)).float(),
                 rbias=(0.1 * u((c.Cout,), 7) + 0.05).float() if c.rbias else None)
    if c.groups:
        t.update(gamma=(1 + 0.2 * u((c.Cin,), 8)).float(), beta=(0.2 * u((c.Cin,), 9)).float())
    return t


def in_stats(x):
    """The producer's integer sums of x: [S][C][2] int64, sum and sum of squares in 2^-24 units (formed in float64)."""
    xd = x.double()
    return torch.stack([torch.round(xd.sum((2, 3)) * 2.0 ** 24), torch.round((xd * xd).sum((2, 3)) * 2.0 ** 24)], -1).to(torch.int64)


def mutant_applies(c, m):
    """drop_half_round  3x3 with a half last round: the wave's last four channels are not summed
    wave_shift       wave 1 reads its input one group of four channels late (3x3; 1x1 with more than one full wave)
    keep_72_79       3x3 with a full round: slots 72-79 keep the weights they loaded (the next 8 floats of the OIHW row) and
                     meet the B value their clamped table entry addresses (channel 7 of the round, tap 8)
    pad_before_gn    3x3 with GroupNorm on load: the halo is normalised like a zero pixel
    up_in_source     the Upsample conv: taps and padding taken on the stored map (conv, then upsample)
    boundary_off     x2 / rx2: channel C1 read behind the first tensor's last channel
    no_rbias         the folded conv's bias omitted"""
    cw = c.Cin >> 3
    if m == "drop_half_round":
        return c.KS == 3 and cw % 8 == 4
    if m == "wave_shift":
        return c.KS == 3 or c.Cin >= 2 * int(_roundup16((c.Cin + 7) // 8)) + 4
    if m == "keep_72_79":
        return c.KS == 3 and cw >= 8
    if m == "pad_before_gn":
        return c.KS == 3 and c.groups > 0
    if m == "up_in_source":
        return c.mode == 2
    if m == "boundary_off":
        return c.C1 > 0 or c.rC1 > 0
    if m == "no_rbias":
        return c.rC > 0 and c.rbias
    raise KeyError(m)


def _gn(x, t, c, dt):
    if dt == torch.float64:
        return cr.gn_forward_f64(x, t["gamma"], t["beta"], bool(c.silu), c.groups)
    y = F.group_norm(x, c.groups, t["gamma"], t["beta"], cr.EPS)
    return F.silu(y) if c.silu else y


def reference(c, t, dt, mutate=None):
    """y of case c in dtype dt (float64: the reference; float32: stock torch on the CPU).  mutate: one of MUTANTS -- the
    same arithmetic with one thing the kernel could get wrong."""
    assert mutate is None or (mutate in MUTANTS and mutant_applies(c, mutate))
    x, w = t["x"].to(dt), t["w"].to(dt).clone()
    cw = c.Cin >> 3
    if mutate == "boundary_off" and c.C1:
        x = x.clone()
        x[:, c.C1] = x.roll(-1, 0)[:, 0]
    if c.groups:
        if mutate == "pad_before_gn":                    # statistics of the map, the affine applied to the halo too
            xg = x.reshape(c.S, c.groups, -1)
            mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
            rep = lambda v: v.repeat_interleave(c.Cin // c.groups, 1)[:, :, None, None]
            xp = F.pad(x, (1, 1, 1, 1))
            xp = (xp - rep(mean)) / torch.sqrt(rep(var) + cr.EPS) * t["gamma"].to(dt)[None, :, None, None] + t["beta"].to(dt)[None, :, None, None]
            x = xp * torch.sigmoid(xp) if c.silu else xp
        else:
            x = _gn(x, t, c, dt)
    if mutate == "drop_half_round":
        for wv in range(8):
            w[:, wv * cw + cw - 4: wv * cw + cw] = 0
    if mutate == "wave_shift":
        x = x.clone()
        if c.KS == 3:
            x[:, cw: 2 * cw] = x[:, cw + 4: 2 * cw + 4].clone()
        else:
            n = int(_roundup16((c.Cin + 7) // 8))
            hi = min(2 * n, c.Cin - 4)
            x[:, n: hi] = x[:, n + 4: hi + 4].clone()
    if mutate == "keep_72_79":
        flat = torch.cat([t["w"].to(dt).reshape(-1), torch.zeros(8, dtype=dt)])
        for wv in range(8):
            for r in range(cw // 8):
                ch = wv * cw + 8 * r + 7
                start = torch.arange(c.Cout) * c.Cin * 9 + (ch + 1) * 9
                w[:, ch, 2, 2] += flat[start[:, None] + torch.arange(8)[None, :]].sum(1)
    pad = 0 if mutate == "pad_before_gn" else c.KS // 2
    if c.mode == 2 and mutate != "up_in_source":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w, t["bias"].to(dt) if c.bias else None, padding=pad)
    if mutate == "up_in_source":
        y = F.interpolate(y, scale_factor=2, mode="nearest")
    if c.vbias:
        y = y + t["vbias"].to(dt)[:, :, None, None]
    if c.residual:
        y = y + t["residual"].to(dt)
    if c.rC:
        rx = t["rx"].to(dt)
        if mutate == "boundary_off":
            rx = rx.clone()
            rx[:, c.rC1] = rx.roll(-1, 0)[:, 0]
        y = y + F.conv2d(rx, t["rw"].to(dt), t["rbias"].to(dt) if (c.rbias and mutate != "no_rbias") else None)
    return y


def tol(c):
    """The family's tolerances: conv outputs 2e-6, behind GroupNorm on load 5e-6."""
    return cr.TOL["small_y"] if c.groups else cr.TOL["small_h"]


def refs(c, t):
    return reference(c, t, torch.float64), reference(c, t, torch.float32)
