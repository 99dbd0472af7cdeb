"""The launch plans of the self-attention block and of the strided batched GEMM beneath it, restated in pure Python:
vf_attention_fwd_kernel and vf_attention_bwd_plan (csrc/attention.hip), vf_bgemm_plan and vf_softmax_plan (csrc/gemm.hip),
the three hand-written block-id -> work maps that place work on one XCD (attn_fwd_q32_kernel, attn_bwd_dvdk_kernel,
bgemm_v2_kernel) with four wrong variants of them, the nine vf_bgemm products of ops.attention / ops.linear, the plan
classes, and the case lists tests/test_gpu_attn_plan.py runs with their inputs and float64 / stock fp32 references.

Class keys (one per independent decision):
  attention forward   ("fwd", kernel, L, C/32 class, placement)   -- every case runs with P written (training) AND with P
                      null (no-grad), so "P written | null" is an axis of the test, not of the case list;
  attention backward  ("bwd", forward kernel that wrote P, route, placement of dscore, dvdk class, C/64 class);
  bgemm               ("bgemm", variant, M tail, N tail, K tail, bias, beta != 0, alpha != 1, batch class, refused terms);
  softmax             ("softmax", MAXV, cols on an edge | ragged against 64, rows % 4)   -- forward and backward both run.
Placement of the 32-query kernel: S < 8 | S % 8 = 0 | S = 8 g + r; of the other kernels: S = 1 | S > 1.  dvdk class: 2 S mod
8 with "2 S < 8" apart.  attention_cases() walks the domain in order of cost and keeps a shape whenever it has a key no
cheaper shape had -- the bgemm classes of the products it launches (key + product name) included: one smallest case per
class; classes whose cheapest shape exceeds ATTN_CAP are over_cap_classes().  There is no single cases(): the three
families take different arguments, so attention_cases(), bgemm_cases() and softmax_cases() stand side by side.
bgemm_cases() holds hand-built views (every variant x tail x epilogue x batch class, each refusal term alone) and, with
ops' own strides and offsets, the three ops.linear products in every class of the sweep S = 1 .. 400 x LIN_SWEEP and the
attention products in the classes the models reach; the attention products of the whole domain run through ops.attention.

Imports no GPU code."""
import collections
import functools
import math

import numpy as np
import torch

import cond_ref as cr

ATTN_CAP = 6e8            # S L^2 C multiply-adds per product of an attention case
BGEMM_CAP = 2e8           # batch M N K of a direct bgemm case
SEED = 71

# vf_attention_fwd_kernel
REFUSED, Q16, Q32, SPLIT, KH = 0, 1, 2, 3, 4
KERNEL_NAMES = {REFUSED: "generic", Q16: "q16", Q32: "q32", SPLIT: "split", KH: "128-query"}
# vf_attention_bwd_plan out[0]
BWD_NONE, BWD_DSCORE_DVDK, BWD_DSCORE_BGEMM, BWD_MATERIALISED = 0, 1, 2, 3
DP, DV, DQ, DK = 1, 2, 4, 8
# vf_bgemm_plan: variant and the refused bits
SLOW, TT, TF, FT, FF = 0, 1, 2, 3, 4
VARIANT_NAMES = ("slow", "TT", "TF", "FT", "FF")
REFUSAL_BITS = ("A no unit stride", "B no unit stride", "sCn != 1", "K % 4", "sAb % 4", "sBb % 4", "sAm % 4", "sAk % 4", "M % 4",
                "sBn % 4", "sBk % 4", "N % 4", "A | B not 16-byte aligned")

SWEEP_S = range(1, 401)
SWEEP_C = (32, 48) + tuple(range(64, 513, 32))
SWEEP_L = (25, 60, 64, 81, 144, 256, 1024, 1296, 4096, 4097)
MAPS = {25: (5, 5), 60: (6, 10), 64: (8, 8), 81: (9, 9), 144: (12, 12), 256: (16, 16), 1024: (32, 32), 1296: (36, 36),
        4096: (64, 64)}


# ------------------------------------------------------------------------------------------------ the planners
def fwd_kernel(S, C, L, q16=True, q32=True):
    """vf_attention_fwd_kernel; q16 / q32: the VF_ATTN_Q16 / VF_ATTN_Q32 tuning aids (read once per process)."""
    if S <= 0 or C <= 0 or C % 32 != 0:
        return REFUSED
    q32_wins = 177 * ((S + 31) // 32) + 30 < 660 * ((S + 127) // 128)
    if L in (256, 64) and S <= 16 and C % 64 == 0 and q16:
        return Q16
    if L == 256 and q32 and q32_wins:
        return Q32
    if L == 256 and S <= 52 and not q32:
        return SPLIT
    if L == 256:
        return KH
    return SPLIT if L == 64 else REFUSED


def fwd_grid(kernel, S, L):
    """(gridDim.x, gridDim.y, threads) of vf_attention_fwd's launch."""
    return {Q16: (L // 16, S, 2 * L), Q32: (8 * S, 1, 256), SPLIT: (L // 32, S, 2 * L), KH: (2, S, 512)}[kernel]


def bwd_plan(S, C, L, dscore=True, dvdk=True):
    """vf_attention_bwd_plan -> [route, dscore workgroups, dvdk workgroups, bgemm products, softmax rows, softmax cols]."""
    if S <= 0 or C <= 0 or L <= 0 or L > 4096:
        return [0] * 6
    ds = bool(dscore) and L == 256 and C % 32 == 0
    dv = ds and bool(dvdk) and C % 64 == 0
    return [1 if dv else 2 if ds else 3, 8 * S if ds else 0, 2 * S * (C // 64) * 2 if dv else 0,
            0 if dv else (DV | DK) if ds else (DP | DV | DQ | DK), 0 if ds else S * L, 0 if ds else L]


def fwd_launches(C, L):
    """ops.attention's forward as C-ABI entries (L <= 4096)."""
    if L in (64, 256) and C % 32 == 0:
        return ["vf_attention_fwd"]
    return ["vf_bgemm", "vf_softmax_fwd", "vf_bgemm"]


def bwd_launches(plan):
    """The C-ABI entries of _AttentionFn.backward, in its order, from a backward plan."""
    route, _, _, prod, rows, _ = plan
    out = ["vf_attention_dscore"] if route in (1, 2) else ["vf_bgemm", "vf_softmax_bwd"]
    if route == 1:
        return out + ["vf_attention_dvdk"]
    return out + ["vf_bgemm"] * (bin(prod & (DV | DQ | DK)).count("1"))


def bgemm_plan(alignA, alignB, batch, M, N, K, sAb, sAm, sAk, sBb, sBk, sBn, sCn, xcd=True):
    """vf_bgemm_plan -> [launches, variant, gx, gy, gz, xcd_batches, refused]; alignA / alignB: the addresses (only their
    low four bits count)."""
    if batch <= 0 or M <= 0 or N <= 0:
        return [0] * 7
    a_kc, a_mc, b_kc, b_nc = sAk == 1, sAm == 1, sBk == 1, sBn == 1
    terms = [not (a_kc or a_mc), not (b_kc or b_nc), sCn != 1, K % 4 != 0, sAb % 4 != 0, sBb % 4 != 0,
             a_kc and sAm % 4 != 0, not a_kc and sAk % 4 != 0, not a_kc and M % 4 != 0,
             b_kc and sBn % 4 != 0, not b_kc and sBk % 4 != 0, not b_kc and N % 4 != 0, ((alignA | alignB) & 15) != 0]
    r = sum(1 << i for i, t in enumerate(terms) if t)
    variant = SLOW if r else (TT if b_kc else TF) if a_kc else (FT if b_kc else FF)
    return [1, variant, (N + 63) // 64, (M + 63) // 64, batch, batch // 8 if xcd else 0, r]


def softmax_maxv(cols):
    return 1 if cols <= 64 else 4 if cols <= 256 else 16 if cols <= 1024 else 64 if cols <= 4096 else 0


def softmax_plan(rows, cols):
    return [softmax_maxv(cols), (rows + 3) // 4 if rows > 0 else 0]


# ------------------------------------------------------------------------------------------------ block id -> work
def q32_map(i, S, mutant=None):
    """attn_fwd_q32_kernel (both roles): block i of 8 S -> (view, query block)."""
    nfull = (S >> 3) << 6
    if mutant == "nfull without << 6":
        nfull = S >> 3
    if i < nfull:
        j = i >> 3
        return ((j >> 3) << 3) + (i & 7), j & 7
    r = i - nfull
    base = (S >> 3) << 3
    if mutant == "remainder base shifted wrongly":
        base = (S >> 3) << 2
    return base + (r >> 3), r & 7


def dvdk_map(i, S, nt, mutant=None):
    """attn_bwd_dvdk_kernel: block i of 2 S nt -> (pair = 2 view + product, tile); nt = 2 C / 64."""
    nfull = ((2 * S) >> 3) << 3
    if i < nfull * nt:
        j = i >> 3
        if mutant == "pair from the wrong quotient":
            return ((j // nt) << 3) + (j & 7), j % nt
        return ((j // nt) << 3) + (i & 7), j % nt
    r = i - nfull * nt
    return nfull + r // nt, r % nt


def bgemm_map(i, gx, gy, batch, xcd_batches, mutant=None):
    """bgemm_v2_kernel: linear block id i = bx + gx (by + gy bz) -> (batch item, tile = by gx + bx)."""
    nt = gx * gy
    if xcd_batches and i < (xcd_batches << 3) * nt:
        j = i >> 3
        if mutant == "tile and b swapped":
            return ((j % nt) << 3) + (i & 7), j // nt
        return ((j // nt) << 3) + (i & 7), j % nt
    return i // nt, i % nt


MUTANTS = {"remainder base shifted wrongly": "q32", "nfull without << 6": "q32", "pair from the wrong quotient": "dvdk",
           "tile and b swapped": "bgemm"}


def map_items(which, n, nt, mutant=None):
    """Every block's work item, in block order; n = S (q32, dvdk) or batch (bgemm), nt = tiles per item (q32: 8)."""
    if which == "q32":
        return [q32_map(i, n, mutant) for i in range(8 * n)]
    if which == "dvdk":
        return [dvdk_map(i, n, nt, mutant) for i in range(2 * n * nt)]
    return [bgemm_map(i, nt, 1, n, n // 8, mutant) for i in range(n * nt)]


def map_faults(which, n, nt, mutant=None):
    """-> list of what is wrong with the map at this size ([] for a sound one): not a bijection onto its work items; an item
    of a whole group of eight whose tiles do not take consecutive slots (i // 8) of ONE XCD (i % 8)."""
    items = map_items(which, n, nt, mutant)
    nitem = 2 * n if which == "dvdk" else n
    want = {(b, t) for b in range(nitem) for t in range(nt)}
    if sorted(items) != sorted(want):
        return ["not a bijection"]
    faults, where = [], collections.defaultdict(list)
    for i, (b, t) in enumerate(items):
        where[b].append((t, i))
    for b in range((nitem >> 3) << 3):
        ids = [i for _, i in sorted(where[b])]
        if {i % 8 for i in ids} != {ids[0] % 8} or [i // 8 for i in ids] != list(range(ids[0] // 8, ids[0] // 8 + nt)):
            faults.append(f"item {b}: not consecutive slots of one XCD")
    return faults


def permuted_views(S, mutant):
    """numpy emulation of a 32-query launch whose blocks copy their (view, query block) of a [S][8] array of distinct
    values: the output under a map (None where a block leaves the array)."""
    src = np.arange(8 * S).reshape(S, 8)
    out = np.full((S, 8), -1)
    for i in range(8 * S):
        b, u = q32_map(i, S, mutant)
        if not 0 <= b < S:
            return None
        out[b, u] = src[b, u]
    return out


# ------------------------------------------------------------------------------------------------ the nine products
Product = collections.namedtuple("Product", "name batch M N K sA sB sC offA offB offC bias alpha")


def attention_products(S, C, L):
    """The six vf_bgemm products ops.attention can run at (S, C, L) (ops/attention.py), offsets in floats into qkv (A of
    qk, pv, dq, dk; B of qk, dp) and dqkv (C of dv, dq, dk)."""
    a, C3 = 1.0 / math.sqrt(C), 3 * C
    return [Product("qk", S, L, L, C, (C3 * L, 1, L), (C3 * L, L, 1), (L * L, L, 1), 0, C * L, 0, False, a),
            Product("pv", S, C, L, L, (C3 * L, L, 1), (L * L, 1, L), (C * L, L, 1), 2 * C * L, 0, 0, False, 1.0),
            Product("dp", S, L, L, C, (C * L, 1, L), (C3 * L, L, 1), (L * L, L, 1), 0, 2 * C * L, 0, False, 1.0),
            Product("dv", S, C, L, L, (C * L, L, 1), (L * L, L, 1), (C3 * L, L, 1), 0, 0, 2 * C * L, False, 1.0),
            Product("dq", S, C, L, L, (C3 * L, L, 1), (L * L, 1, L), (C3 * L, L, 1), C * L, 0, 0, False, a),
            Product("dk", S, C, L, L, (C3 * L, L, 1), (L * L, L, 1), (C3 * L, L, 1), 0, 0, C * L, False, a)]


def linear_products(S, I, O):
    """The three vf_bgemm products of ops.linear (ops/dense.py): y = x w^T + b, dx = dy w, dw = dy^T x."""
    return [Product("lin", 1, S, O, I, (0, I, 1), (0, 1, I), (0, O, 1), 0, 0, 0, True, 1.0),
            Product("lin dx", 1, S, I, O, (0, O, 1), (0, I, 1), (0, I, 1), 0, 0, 0, False, 1.0),
            Product("lin dw", 1, O, I, S, (0, 1, O), (0, I, 1), (0, I, 1), 0, 0, 0, False, 1.0)]


def product_plan(p):
    """The bgemm plan of a product on 16-byte aligned tensors."""
    return bgemm_plan(4 * p.offA, 4 * p.offB, p.batch, p.M, p.N, p.K, *p.sA, *p.sB, p.sC[2])


def products_run(S, C, L, dscore=True, dvdk=True):
    """The products a training call of ops.attention launches at (S, C, L), by name."""
    names = [] if fwd_launches(C, L) == ["vf_attention_fwd"] else ["qk", "pv"]
    prod = bwd_plan(S, C, L, dscore, dvdk)[3]
    return names + [n for n, bit in (("dp", DP), ("dv", DV), ("dq", DQ), ("dk", DK)) if prod & bit]


# ------------------------------------------------------------------------------------------------ class keys
def c32_class(C):
    n = C // 32
    return "10" if n == 10 else str(n) if n <= 2 else "odd >= 3" if n % 2 else "even >= 4"


def placement(kernel, S):
    if kernel == Q32:
        return "S < 8" if S < 8 else "S % 8 = 0" if S % 8 == 0 else "S = 8g + r"
    return "S = 1" if S == 1 else "S > 1"


def batch_class(b):
    return "1" if b == 1 else "< 8" if b < 8 else "8g" if b % 8 == 0 else "8g + r"


def refusal_names(r):
    return tuple(n for i, n in enumerate(REFUSAL_BITS) if r >> i & 1)


def fwd_key(S, C, L):
    k = fwd_kernel(S, C, L) if L in (64, 256) else REFUSED
    return ("fwd", KERNEL_NAMES[k], L, c32_class(C) if k else f"C % 32 = {C % 32}", placement(k, S))


def bwd_key(S, C, L, dscore=True, dvdk=True):
    k = fwd_kernel(S, C, L) if L in (64, 256) else REFUSED
    route = bwd_plan(S, C, L, dscore, dvdk)[0]
    if route == BWD_MATERIALISED:
        name = "generic" if not k else "round-4 route" if L == 256 else "L = 64"
        return ("bwd", KERNEL_NAMES[k], name, batch_class(S), None, None)
    dv = None if route != 1 else (f"2S = {2 * S} < 8" if 2 * S < 8 else f"2S % 8 = {2 * S % 8}")
    return ("bwd", KERNEL_NAMES[k], "dscore+dvdk" if route == 1 else "dscore+2 bgemm", placement(Q32, S), dv,
            None if route != 1 else str(C // 64) if C // 64 < 3 else ">= 3")


def bgemm_key(plan, M, N, K, bias, beta, alpha):
    ktail = "K % 32 = 0" if K % 32 == 0 else "K % 4 = 0" if K % 4 == 0 else "K % 4 != 0"
    return ("bgemm", VARIANT_NAMES[plan[1]], "M tail" if M % 64 else "M full", "N tail" if N % 64 else "N full", ktail,
            "bias" if bias else "no bias", "beta" if beta != 0 else "beta 0", "alpha" if alpha != 1 else "alpha 1",
            batch_class(plan[4]), refusal_names(plan[6]))


def product_key(p):
    return bgemm_key(product_plan(p), p.M, p.N, p.K, p.bias, 0.0, p.alpha)


def softmax_key(rows, cols):
    return ("softmax", softmax_maxv(cols), "edge" if cols % 64 == 0 else "ragged", rows % 4)


# ------------------------------------------------------------------------------------------------ attention cases
ACase = collections.namedtuple("ACase", "S C H W dscore dvdk why")
FLAGS = ((1, 1), (1, 0), (0, 1))       # (st.ATTN_DSCORE, st.ATTN_DVDK): default, dscore + products, the round-4 route
GENERIC_S = (1, 3, 8, 11)


def a_id(c):
    return f"S{c.S}-C{c.C}-{c.H}x{c.W}" + ("" if c.dscore else "-nodscore") + ("" if c.dvdk else "-nodvdk")


def a_cost(S, C, L):
    return S * L * L * C


def a_keys(S, C, L, dscore=1, dvdk=1):
    """The forward, backward and product (bgemm) keys of a training call."""
    byname = {p.name: p for p in attention_products(S, C, L)}
    return [fwd_key(S, C, L), bwd_key(S, C, L, dscore, dvdk)] + \
           [product_key(byname[n]) + (n,) for n in products_run(S, C, L, dscore, dvdk)]


def _domain():
    """(cost, S, C, L, dscore, dvdk) of every shape the enumeration looks at: the fused maps with every C % 32 = 0 of the
    sweep, and the issue's generic maps (9x9, 6x10, 32x32, 12x12 at C = 48, 64x64 at S = 1)."""
    out = []
    for L in (64, 256):
        for C in (c for c in SWEEP_C if c % 32 == 0):
            for S in SWEEP_S:
                for ds, dv in FLAGS if L == 256 else FLAGS[:1]:
                    if dv or C % 64 == 0:                          # (the dvdk switch matters only where dvdk applies)
                        out.append((a_cost(S, C, L), S, C, L, ds, dv))
    for L, C, Ss in ((81, 32, GENERIC_S), (60, 32, GENERIC_S), (1024, 32, GENERIC_S), (144, 48, GENERIC_S), (4096, 32, (1,))):
        out += [(a_cost(S, C, L), S, C, L, 1, 1) for S in Ss]
    return sorted(out, key=lambda t: (t[0], t[1], t[2], t[3], -t[4], -t[5]))


# the S edges of the forward's cost rule and of the 16-query kernel, both sides (the issue's list), at the cheapest C
EDGES = ((16, 64), (17, 64), (96, 32), (97, 32), (128, 32), (129, 32), (224, 32), (225, 32))


@functools.lru_cache(None)
def _enumerate():
    """-> (cases, covered keys, {key over the cap: its cheapest shape})."""
    cases, covered, over = [], set(), {}
    for cost, S, C, L, ds, dv in _domain():
        keys = [k for k in a_keys(S, C, L, ds, dv) if k not in covered]          # (the products' bgemm classes count too)
        if not keys:
            continue
        if cost > ATTN_CAP:
            for k in keys:
                over.setdefault(k, (S, C, L, ds, dv))
            continue
        covered.update(a_keys(S, C, L, ds, dv))
        cases.append(ACase(S, C, *MAPS[L], ds, dv, "; ".join(" ".join(", ".join(v) if isinstance(v, tuple) else str(v) for v in k[1:] if v not in (None, ()))
                                                           for k in keys)))
    for S, C in EDGES:
        c = ACase(S, C, 16, 16, 1, 1, f"edge of the forward's choice: S = {S}")
        if c[:6] not in {x[:6] for x in cases}:
            assert a_cost(S, C, 256) <= ATTN_CAP
            cases.append(c)
            covered.update(a_keys(S, C, 256))
    return tuple(cases), frozenset(covered), {k: v for k, v in over.items() if k not in covered}


def attention_cases():
    return list(_enumerate()[0])


def attention_covered():
    return set(_enumerate()[1])


def over_cap_classes():
    return dict(_enumerate()[2])


def model_attention_shapes():
    """(C, L) of every self-attention block of the SMALL and TINY networks (view_fusion_amd/unet.py), and (I, O) of their
    embedding MLP's two linears."""
    from conftest import SMALL, TINY
    from view_fusion_amd import UNet
    attn, lin = set(), set()
    for hp in (SMALL, TINY):
        net = UNet(**hp)
        for layer in list(net.downs) + list(net.mid) + list(net.ups):
            if getattr(layer, "attn", None) is not None:
                H = hp["image_size"] >> layer.res_block.block1["block"]["3"]._vf_geom[0]
                attn.add((layer.attn.norm.num_channels, H * H))
        for k in ("0", "2"):
            w = net.noise_level_mlp[k].weight
            lin.add((w.shape[1], w.shape[0]))
    return sorted(attn), sorted(lin)


MODEL_S = range(1, 369)
LIN_SWEEP = tuple((i, o) for i in (32, 64, 128, 256) for o in (32, 64, 128, 256))       # (I, O) of ops.linear in the sweep


def domain_bgemm_classes():
    """{bgemm key + product name: first shape} of every product the attention domain (_domain) and the linear sweep
    (S = 1 .. 400 x LIN_SWEEP) launch: each must have a case or be named over the cap."""
    reached = {}
    for _, S, C, L, ds, dv in _domain():
        for k in a_keys(S, C, L, ds, dv):
            if k[0] == "bgemm":
                reached.setdefault(k, (S, C, L))
    for S in SWEEP_S:
        for I, O in LIN_SWEEP:
            for p in linear_products(S, I, O):
                reached.setdefault(product_key(p) + (p.name,), (S, I, O))
    return reached


def model_classes():
    """{key: first S that reaches it} over the SMALL / TINY attention blocks and linears at S = 1 .. 368."""
    attn, lin = model_attention_shapes()
    reached = {}
    for S in MODEL_S:
        for C, L in attn:
            for k in a_keys(S, C, L):
                reached.setdefault(k, (S, C, L))
        for I, O in lin:
            for p in linear_products(S, I, O):
                reached.setdefault(product_key(p) + (p.name,), (S, I, O))
    return reached


def attn_tensors(c):
    """-> (qkv (S, 3C, L), dy (S, C, L)) float32: cond_ref.attn_input at scale 2, shift 0 (every view different)."""
    L = c.H * c.W
    return cr.attn_input(c.S, c.C, L, 2, 0, SEED), cr._u((c.S, c.C, L), SEED + 7).float()


# ------------------------------------------------------------------------------------------------ direct bgemm cases
BCase = collections.namedtuple("BCase", "name batch M N K sA sB sC offA offB offC bias alpha beta why")


def _layout(kind, rows, cols, pad):
    """(row stride, col stride, floats) of one [rows][cols] matrix: kind "r" cols contiguous, "c" rows contiguous, "2" no
    unit stride (every fourth float, so that nothing else of the fast predicate fails); pad: extra floats on the leading
    dimension."""
    if kind == "r":
        return cols + pad, 1, rows * (cols + pad)
    if kind == "c":
        return 1, rows + pad, cols * (rows + pad)
    return 4 * (cols + pad), 4, 4 * rows * (cols + pad)


def mk_b(name, batch, M, N, K, a="r", b="r", padA=0, padB=0, gapA=0, gapB=0, offA=0, offB=0, sCn=1, bias=False, alpha=1.0,
         beta=0.0, why=""):
    """A direct case on strided views: A[m][k] laid out by `a` ("r": k contiguous), B[k][n] by `b` ("r": n contiguous)."""
    sAm, sAk, nA = _layout(a, M, K, padA)
    sBk, sBn, nB = _layout(b, K, N, padB)
    return BCase(name, batch, M, N, K, (nA + gapA, sAm, sAk), (nB + gapB, sBk, sBn), (M * (N + 3) * sCn + 8, (N + 3) * sCn, sCn),
                 offA, offB, 4, bias, alpha, beta, why)


def from_product(p, why):
    return BCase(p.name, p.batch, p.M, p.N, p.K, p.sA, p.sB, p.sC, p.offA, p.offB, p.offC, p.bias, p.alpha, 0.0, why)


def b_plan(c):
    return bgemm_plan(4 * c.offA, 4 * c.offB, c.batch, c.M, c.N, c.K, *c.sA, *c.sB, c.sC[2])


def b_key(c):
    return bgemm_key(b_plan(c), c.M, c.N, c.K, c.bias, c.beta, c.alpha)


PRODUCT_NAMES = ("qk", "pv", "dp", "dv", "dq", "dk", "lin", "lin dx", "lin dw")


def b_named_key(c):
    """b_key + the product of ops whose arguments the case carries ("direct": a hand-built view) -- the form of the keys
    a_keys gives the products of an attention case."""
    return b_key(c) + (c.name if c.name in PRODUCT_NAMES else "direct",)


def b_id(c):
    return f"{c.name}-b{c.batch}-{c.M}x{c.N}x{c.K}"


_LAYOUTS = {TT: ("r", "c"), TF: ("r", "r"), FT: ("c", "c"), FF: ("c", "r")}


@functools.lru_cache(None)
def _bgemm_cases():
    out = []
    for v, (a, b) in _LAYOUTS.items():
        n = VARIANT_NAMES[v]
        # every tail at once, more than one tile each way, epilogue terms on, whole groups of eight and a remainder
        out.append(mk_b(f"{n} tails", 11, 68, 72, 36, a, b, padA=4, padB=8, gapA=4, gapB=8, offA=4, offB=8, bias=True, alpha=0.5,
                        beta=0.25, why="M, N mod 64 and K mod 32 tails, 2 x 2 tiles, bias, alpha, beta, batch 8g + r"))
        out.append(mk_b(f"{n} full", 8, 64, 128, 64, a, b, why="no tail, two K chunks, batch 8g, plain epilogue"))
        out.append(mk_b(f"{n} few", 3, 4, 8, 4, a, b, bias=True, why="one partly filled tile, K = 4, batch < 8"))
        out.append(mk_b(f"{n} one", 1, 128, 60, 32, a, b, beta=-1.5, why="batch 1, N tail only, beta alone"))
    for a, b in (("r", "c"), ("r", "r"), ("c", "c"), ("c", "r")):
        tag = a + b
        out.append(mk_b(f"slow {tag} tails", 11, 67, 70, 37, a, b, padA=1, padB=3, gapA=1, offA=1, offB=2, bias=True, alpha=0.5,
                        beta=0.25, why="the slow kernel's four staging orders: every tail, K % 4 != 0, batch 8g + r"))
    out.append(mk_b("slow full", 8, 64, 64, 32, "2", "r", why="slow kernel without a tail (A has no unit stride), batch 8g"))
    out.append(mk_b("slow few", 3, 5, 7, 3, "r", "r", why="K < 4, batch < 8"))
    out.append(mk_b("slow one", 1, 65, 1, 33, "c", "c", alpha=-2.0, why="N = 1, batch 1"))
    # each term of the fast predicate failing ALONE (the library confirms: refused has exactly that bit)
    solo = [mk_b("no A unit", 2, 8, 8, 8, "2", "r"), mk_b("no B unit", 2, 8, 8, 8, "r", "2"), mk_b("sCn", 2, 8, 8, 8, sCn=2),
            mk_b("K4", 2, 8, 8, 6, "c", "r"), mk_b("sAb4", 2, 8, 8, 8, gapA=2), mk_b("sBb4", 2, 8, 8, 8, gapB=2),
            mk_b("sAm4", 2, 8, 8, 8, "r", "r", padA=1, gapA=8), mk_b("sAk4", 2, 8, 8, 8, "c", "r", padA=2, gapA=16),
            mk_b("M4", 2, 6, 8, 8, "c", "r", padA=2, gapA=0), mk_b("sBn4", 2, 8, 8, 8, "r", "c", padB=1, gapB=8),
            mk_b("sBk4", 2, 8, 8, 8, "r", "r", padB=2, gapB=16), mk_b("N4", 2, 8, 6, 8, "r", "r", padB=2, gapB=0),
            mk_b("align A", 2, 8, 8, 8, offA=1), mk_b("align B", 2, 8, 8, 8, offB=2)]
    for c in solo:
        out.append(c._replace(name="refused " + c.name, why="one term of the fast predicate fails alone"))
    # the products of ops.linear over the whole sweep and of ops.attention in the classes the models reach, with ops' own
    # strides and offsets: one case per (class, product).  (The attention products of the whole domain run through
    # ops.attention: attention_cases() counts their classes.)
    have = set()
    attn, _ = model_attention_shapes()
    for S in SWEEP_S:
        ps = [p for C, L in attn for p in attention_products(S, C, L) if p.name in products_run(S, C, L)] if S in MODEL_S else []
        ps += [p for I, O in LIN_SWEEP for p in linear_products(S, I, O)]
        for p in ps:
            k = product_key(p) + (p.name,)
            if k not in have and p.batch * p.M * p.N * p.K <= BGEMM_CAP:
                have.add(k)
                out.append(from_product(p, f"{p.name} with the arguments ops passes, first at S = {S}"))
    return tuple(out)


def bgemm_cases():
    return list(_bgemm_cases())


def b_tensors(c):
    """-> (bufA, bufB, bufC (pre-filled), bias | None) float32, each just large enough for the case's views."""
    ext = lambda off, s, dims: off + sum((d - 1) * abs(x) for d, x in zip(dims, s)) + 1
    nA, nB = ext(c.offA, c.sA, (c.batch, c.M, c.K)), ext(c.offB, c.sB, (c.batch, c.K, c.N))
    nC = ext(c.offC, c.sC, (c.batch, c.M, c.N))
    return (cr._u((nA + 3,), SEED + 1).float(), cr._u((nB + 3,), SEED + 2).float(), cr._u((nC,), SEED + 3).float(),
            cr._u((c.N,), SEED + 4).float() if c.bias else None)


def b_index(off, s, dims):
    i = [torch.arange(d, dtype=torch.int64) for d in dims]
    return off + i[0][:, None, None] * s[0] + i[1][None, :, None] * s[1] + i[2][None, None, :] * s[2]


def b_ref(c, A, B, Cbuf, bias, dt):
    """The contraction on the gathered views in dtype dt -> the [batch][M][N] result (beta on the pre-filled C)."""
    a = A[b_index(c.offA, c.sA, (c.batch, c.M, c.K))].to(dt)
    b = B[b_index(c.offB, c.sB, (c.batch, c.K, c.N))].to(dt)
    r = c.alpha * torch.bmm(a, b)
    if bias is not None:
        r = r + bias.to(dt)[None, None, :]
    if c.beta != 0:
        r = r + c.beta * Cbuf[b_index(c.offC, c.sC, (c.batch, c.M, c.N))].to(dt)
    return r


# ------------------------------------------------------------------------------------------------ softmax cases
SOFTMAX_COLS = {(1, "edge"): (64, 64, 64, 64), (1, "ragged"): (1, 37, 63, 5), (4, "edge"): (256, 128, 192, 256),
                (4, "ragged"): (65, 200, 255, 129), (16, "edge"): (1024, 320, 512, 1024), (16, "ragged"): (257, 1000, 1023, 700),
                (64, "edge"): (4096, 1088, 2048, 4096), (64, "ragged"): (1025, 4000, 4095, 2500)}     # by rows % 4
SOFTMAX_ROWS = (8, 5, 6, 7)         # rows % 4 = 0, 1, 2, 3: two workgroups, the second one partly filled
SOFTMAX_SCALE = 6.0


def softmax_cases():
    """(rows, cols): one per (MAXV, edge | ragged, rows % 4); the forward and the backward both run on each."""
    return [(SOFTMAX_ROWS[r], cols[r]) for (_, _), cols in sorted(SOFTMAX_COLS.items()) for r in range(4)]


def softmax_tensors(rows, cols):
    """-> (x, y = float64 softmax rounded once, dy) float32."""
    x = (SOFTMAX_SCALE * cr._u((rows, cols), SEED + 5)).float()
    return x, torch.softmax(x.double(), -1).float(), cr._u((rows, cols), SEED + 6).float()


def softmax_refs(x, y, dy):
    """-> (r64, r32): each [softmax(x), y o (dy - rowsum(y o dy))]."""
    def run(dt):
        yy, dd = y.to(dt), dy.to(dt)
        return [torch.softmax(x.to(dt), -1), yy * (dd - (yy * dd).sum(-1, keepdim=True))]
    return run(torch.float64), run(torch.float32)


def softmax_floor():
    """Four times the largest stock fp32 error over the case list, rounded up to one digit: cond_ref.TOL["softmax"]."""
    e = max(cr.err(a, b) for rows, cols in softmax_cases()
            for r64, r32 in [softmax_refs(*softmax_tensors(rows, cols))] for a, b in zip(r32, r64))
    x = 4 * e
    p = 10.0 ** math.floor(math.log10(x))
    return e, math.ceil(x / p - 1e-9) * p
