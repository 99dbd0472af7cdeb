"""The launch plan of the streaming self-attention kernels (csrc/attention_stream.hip: attn_stream_plan, which
vf_attn_stream_fwd / vf_attn_stream_bwd execute and vf_attn_stream_plan reports) restated in pure Python, the index algebra
of the kernels restated in numpy (crow, put_tile, chan_mfma, the waves' channel tiles, ld4, block_ids with three wrong
variants of the remap), a numpy model of the algorithm as written with eight wrong variants of it, the plan classes, and
the case list tests/test_gpu_attn_stream_plan.py runs with its inputs and float64 / stock fp32 references.

Class keys (one per independent decision; a case is kept whenever it has a key no cheaper shape had):
  ("chan", NT, last tile full | partial, waves: all equal | some without a tile | unequal counts,
           tail: C % 16 = 0 | even tail | odd C, size: C = 1 | C < 16 | C >= 16)
  ("vec", NT, state)      state: "1/1" | "0/0 L % 4 = 1" | "... = 2" | "... = 3" | "0/0 qkv misaligned" | "1/0 dO misaligned"
                          (forward / backward; every <NT> instantiation has its own copy of ld4)
  ("L", special, blocks, live sub-blocks of the last block, last live sub-block ragged | whole)
                          special: "L = 1" | "L < 32" | "L = 32" | "L = 128" | "L = 129" | None; blocks: 1 | 2 | 3 | ">= 4".
                          With one block, 4 - live is the number of dead sub-blocks of the FIRST block (the
                          mw == -inf branch while m is still -inf); "ragged" is also "the last query block is partly
                          stored" (queries and keys share L).
  ("blocks", NT, blocks)  the rescale of the O accumulators and the LDS buffer reuse, per instantiation
  ("grid", S = 1 | S > 1, workgroups < 8 | % 8 = 0 | % 8 != 0)
rowstat present | NULL is an axis of the test (every case runs both), not of the list.

cases(): 100 cases for 115 keys, none over ATTN_CAP (tests/test_attn_stream_plan_host.py asserts both numbers).

Imports no GPU code."""
import collections
import functools
import math

import numpy as np
import torch

import cond_ref as cr
from attn_plan_ref import ATTN_CAP

SEED = 83
LOG2E = 1.4426950408889634
EMPTY, RUNS, REFUSED = 0, 1, 2
FIELDS = ("state", "NT", "vec_fwd", "vec_bwd", "gx", "gy", "delta_gx", "nblocks", "rowstat_floats", "delta_floats")
INT_MAX = 2 ** 31 - 1
SQ, SKB, SPAD = 32, 128, 36


# ------------------------------------------------------------------------------------------------ the plan
def tiles_per_wave(C):
    return ((C + 31) // 32 + 3) // 4


def plan(align_qkv, align_dO, S, C, L):
    """vf_attn_stream_plan -> the ten ints of FIELDS; align_*: the addresses (only their low four bits count)."""
    if S <= 0 or L <= 0:
        return [EMPTY] + [0] * 9
    if C <= 0 or C > 512:
        return [REFUSED] + [0] * 9
    vf = int(L % 4 == 0 and align_qkv % 16 == 0)
    return [RUNS, tiles_per_wave(C), vf, int(vf and align_dO % 16 == 0), (L + 31) // 32, S, (L + 255) // 256, (L + 127) // 128,
            min(2 * S * L, INT_MAX), min(S * L, INT_MAX)]


def plan_arrays(aq, ad, S, C, L):
    """plan() on int64 arrays (broadcast together) -> (..., 10) int64."""
    aq, ad, S, C, L = np.broadcast_arrays(*(np.asarray(a, dtype=np.int64) for a in (aq, ad, S, C, L)))
    empty = (S <= 0) | (L <= 0)
    refused = ~empty & ((C <= 0) | (C > 512))
    run = ~empty & ~refused
    vf = (L % 4 == 0) & (aq % 16 == 0)
    cols = [np.where(empty, EMPTY, np.where(refused, REFUSED, RUNS)), ((C + 31) // 32 + 3) // 4, vf, vf & (ad % 16 == 0),
            (L + 31) // 32, S, (L + 255) // 256, (L + 127) // 128, np.minimum(2 * S * L, INT_MAX), np.minimum(S * L, INT_MAX)]
    out = np.stack([np.asarray(c, dtype=np.int64) for c in cols], -1)
    out[..., 1:] *= run[..., None]
    return out


# ------------------------------------------------------------------------------------------------ the index algebra
def crow(r, lh):
    """Accumulator register r of lane half lh of v_mfma_f32_32x32x2_f32 -> its row."""
    return (r & 3) + 8 * (r >> 2) + 4 * lh


def put_tile_column(g, e, lh):
    """put_tile: where register 4 g + e of lane half lh lands in the LDS row."""
    return 8 * g + 4 * lh + e


def tiles_read_column(g, e, lh):
    """chan_tiles_mfma: the LDS column MFMA step (g, e) of lane half lh reads as its B value -- the key (query) it pairs
    with the A value ld4 fetched at kbase + 32 u + 8 g + 4 lh + e."""
    return 8 * g + 4 * lh + e


def chan_mfma_channels(C, mutant=None):
    """chan_mfma -> (channels summed, one entry per (MFMA step, lane half) that is not masked; channels whose address is
    formed, masked steps included)."""
    summed, addressed = [], []
    c0 = 0
    while c0 + 16 <= C:
        for j in range(8):
            for lh in (0, 1):
                summed.append(c0 + 2 * j + lh)
                addressed.append(c0 + 2 * j + lh)
        c0 += 16
    while c0 + 2 <= C if mutant == "the last odd channel dropped" else c0 < C:
        for lh in (0, 1):
            c = c0 + lh
            addressed.append(c if c < C else 0)
            if c < C:
                summed.append(c)
        c0 += 2
    return summed, addressed


def wave_tiles(C):
    """-> [tiles of wave 0, .., of wave 3]: w + 4 t for t < NT while 32 (w + 4 t) < C (chan_tiles_mfma and the stores)."""
    nt = tiles_per_wave(C)
    return [[w + 4 * t for t in range(nt) if 32 * (w + 4 * t) < C] for w in range(4)]


def ld4_addresses(kk, L, vec):
    """ld4 -> (the four offsets into the row it reads, whether it reads them as one 16-byte load)."""
    if vec and kk < L:
        return [kk, kk + 1, kk + 2, kk + 3], True
    return [min(kk + t, L - 1) for t in range(4)], False


def ld4_kk(L):
    """Every kk chan_tiles_mfma passes to ld4 at this L: kbase + 32 u + 8 g + 4 lh over all 128-wide blocks."""
    return [128 * kb + 32 * u + 8 * g + 4 * lh for kb in range((L + 127) // 128) for u in range(4) for g in range(4) for lh in (0, 1)]


REMAP_MUTANTS = ("start without the remainder", "xcd and slot swapped", "blk and b by gridDim.y")


def xcd_remap(bid, nblk, mutant=None):
    """common.h: physical block bid (XCD bid % 8, slot bid / 8) -> logical id; numpy arrays or ints."""
    q, r = nblk >> 3, nblk & 7
    xcd, slot = bid & 7, bid >> 3
    if mutant == "xcd and slot swapped":
        return xcd + 8 * slot
    if mutant == "start without the remainder":
        return xcd * q + slot
    return np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + slot


def block_ids(gx, gy, mutant=None):
    """block_ids for every physical block of a (gx, gy) grid, in launch order bx + gx by -> (blk, b) int64 arrays."""
    nb = gx * gy
    ids = xcd_remap(np.arange(nb, dtype=np.int64), nb, mutant)
    if mutant == "blk and b by gridDim.y":
        return ids % gy, ids // gy
    return ids % gx, ids // gx


def block_ids_faults(gx, gy, mutant=None):
    """-> what is wrong with block_ids at this grid ([] for a sound one): not a bijection onto (block < gx, view < gy); an
    XCD whose blocks do not take consecutive logical ids in slot order (blocks i, i + 8, .. share an XCD: consecutive
    logical ids must share one, so that a view's blocks share an L2)."""
    blk, b = block_ids(gx, gy, mutant)
    nb = gx * gy
    if blk.min() < 0 or blk.max() >= gx or b.min() < 0 or b.max() >= gy or np.unique(b * gx + blk).size != nb:
        return ["not a bijection"]
    logical = b * gx + blk
    for x in range(min(8, nb)):
        mine = logical[x::8]
        if mine.size > 1 and not (np.diff(mine) == 1).all():
            return [f"XCD {x}: its blocks do not take consecutive logical ids"]
    return []


def remap_intervals_tile(nb_max):
    """For every nb <= nb_max at once: XCD x holds count_x = nb / 8 (+ 1 if x < nb % 8) physical blocks and maps them onto
    [start_x, start_x + count_x); the map is a bijection of [0, nb) iff those eight intervals tile it in order."""
    nb = np.arange(1, nb_max + 1, dtype=np.int64)[:, None]
    x = np.arange(8, dtype=np.int64)[None, :]
    q, r = nb >> 3, nb & 7
    count = q + (x < r)
    start = np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q)
    return bool((start[:, :1] == 0).all() and (start[:, 1:] == (start + count)[:, :-1]).all() and ((start + count)[:, 7:] == nb).all())


# ------------------------------------------------------------------------------------------------ the model
FWD_MUTANTS = ("no rescale of O when the running maximum rises", "a dead sub-block contributing exp2(0) = 1", "masked keys scored 0",
               "the ragged last block dropped", "the last odd channel dropped")
BWD_MUTANTS = ("dS without -delta", "statistics of the last block instead of the running ones", "dK without alpha")
MUTANTS = FWD_MUTANTS + BWD_MUTANTS


def mutant_applies(mutant, S, C, L):
    """Whether a wrong model differs from the right one at this shape (the host test asserts it then fails the rule)."""
    nblocks, tail = (L + 127) // 128, L % 128
    return {"no rescale of O when the running maximum rises": nblocks >= 2 and L >= 10 and C >= MIN_C,      # (attn_input puts a largest key last)
            "a dead sub-block contributing exp2(0) = 1": 0 < tail <= 96,
            "masked keys scored 0": L % 32 != 0,
            "the ragged last block dropped": tail != 0,
            "the last odd channel dropped": C % 2 == 1 and L >= 2,                            # (one key: p = 1 whatever it scores)
            "dS without -delta": True,
            "statistics of the last block instead of the running ones": nblocks >= 2,
            "dK without alpha": C > 1 and L >= 2}[mutant]                                      # (one key: dS = 0)


def _scores(q, k, C, mutant):
    ch = chan_mfma_channels(C, mutant)[0]
    return q[ch].T @ k[ch]                                   # raw scores [query][key]; c2 carries alpha


def model_forward(qkv, mutant=None):
    """The forward as written, in float64: 128-key blocks, one 32-key sub-block per wave, keys past L at -inf, a sub-block
    wholly past L contributing 0, the four sub-blocks' statistics combined in wave order, O rescaled by the rise of the
    running maximum -> (out (S, C, L), rowstat (S, 2, L) = (c2 max, 1 / sum))."""
    x = qkv.double().numpy()
    S, C3, L = x.shape
    C = C3 // 3
    c2 = LOG2E / math.sqrt(C)
    nkb = (L + SKB - 1) // SKB
    out, stat = np.empty((S, C, L)), np.empty((S, 2, L))
    for b in range(S):
        q, k, v = x[b].reshape(3, C, L)
        sp = np.full((L, nkb * SKB), -np.inf)
        sp[:, :L] = _scores(q, k, C, mutant)
        vp = np.zeros((C, nkb * SKB))
        vp[:, :L] = v                                        # (ld4: entries at or past L read as 0)
        m, l, o = np.full(L, -np.inf), np.zeros(L), np.zeros((L, C))
        for kb in range(L // SKB if mutant == "the ragged last block dropped" else nkb):
            mu, lw, pu = [], [], []
            for u in range(4):
                k0 = kb * SKB + 32 * u
                sub = sp[:, k0:k0 + 32].copy()
                if mutant == "masked keys scored 0" and k0 < L < k0 + 32:
                    sub[:, L - k0:] = 0.0
                mw = sub.max(1)
                dead = np.isneginf(mw)
                with np.errstate(invalid="ignore"):
                    p = np.exp2(sub * c2 - np.where(dead, 0.0, mw * c2)[:, None])
                if mutant == "a dead sub-block contributing exp2(0) = 1" and k0 >= L:
                    p, mw = np.ones_like(sub), np.zeros(L)
                mu.append(mw)
                lw.append(p.sum(1))
                pu.append(p)
            mn = np.maximum.reduce([m] + mu)
            fo = np.exp2((m - mn) * c2)                      # m = -inf on the first block: 0
            l = l * fo
            o = o * (1.0 if mutant == "no rescale of O when the running maximum rises" else fo[:, None])
            for u in range(4):
                f = np.exp2((mu[u] - mn) * c2)
                l = l + f * lw[u]
                o = o + (pu[u] * f[:, None]) @ vp[:, kb * SKB + 32 * u:kb * SKB + 32 * u + 32].T
            m = mn
            last = (mu, lw)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = (o / l[:, None]).T
            if mutant == "statistics of the last block instead of the running ones":
                m = np.maximum.reduce(last[0])
                l = sum(np.exp2((a - m) * c2) * w for a, w in zip(*last))
            stat[b, 0], stat[b, 1] = m * c2, 1.0 / l
    return torch.from_numpy(out), torch.from_numpy(stat)


def model_backward(qkv, out, dO, rowstat, mutant=None):
    """The backward as written, in float64: delta = rowsum(dO o out), p = exp2(c2 s - c2 max) / sum recomputed from the
    saved pair, -delta the initial accumulator of dP, dS = p o dP', dK and dQ scaled by alpha -> dqkv (S, 3C, L)."""
    x, o, g, st = (t.double().numpy() for t in (qkv, out, dO, rowstat))
    S, C3, L = x.shape
    C = C3 // 3
    alpha = 1.0 / math.sqrt(C)
    c2 = LOG2E * alpha
    dx = np.empty((S, 3, C, L))
    for b in range(S):
        q, k, v = x[b].reshape(3, C, L)
        delta = (g[b] * o[b]).sum(0)
        with np.errstate(invalid="ignore"):                  # (a wrong forward may hand over NaN; the rule then fails it)
            p = np.exp2(_scores(q, k, C, mutant) * c2 - st[b, 0][:, None]) * st[b, 1][:, None]
            dp = g[b].T @ v - (0.0 if mutant == "dS without -delta" else delta[:, None])
            ds = p * dp
            dx[b, 0] = alpha * (k @ ds.T)
            dx[b, 1] = (1.0 if mutant == "dK without alpha" else alpha) * (q @ ds)
            dx[b, 2] = g[b] @ p
    return torch.from_numpy(dx.reshape(S, C3, L))


def model(qkv, dO, mutant=None):
    """-> [out, dqkv, rowstat] of the model (a forward mutant feeds its own out and rowstat to the backward, as the
    kernels would)."""
    out, stat = model_forward(qkv, mutant if mutant in FWD_MUTANTS or mutant == BWD_MUTANTS[1] else None)
    return [out, model_backward(qkv, out, dO, stat, mutant), stat]


# ------------------------------------------------------------------------------------------------ class keys
def chan_key(C):
    nt, tiles = tiles_per_wave(C), (C + 31) // 32
    waves = "some without a tile" if tiles < 4 else "all equal" if tiles % 4 == 0 else "unequal counts"
    tail = "C % 16 = 0" if C % 16 == 0 else "even tail" if C % 2 == 0 else "odd C"
    return ("chan", nt, "last tile full" if C % 32 == 0 else "last tile partial", waves, tail,
            "C = 1" if C == 1 else "C < 16" if C < 16 else "C >= 16")


VEC_STATES = ("1/1", "0/0 L % 4 = 1", "0/0 L % 4 = 2", "0/0 L % 4 = 3", "0/0 qkv misaligned", "1/0 dO misaligned")


def vec_state(aq, ad, L):
    if L % 4:
        return f"0/0 L % 4 = {L % 4}"
    return "0/0 qkv misaligned" if aq % 16 else "1/0 dO misaligned" if ad % 16 else "1/1"


def blocks_class(L):
    n = (L + 127) // 128
    return str(n) if n < 4 else ">= 4"


def l_key(L):
    special = {1: "L = 1", 32: "L = 32", 128: "L = 128", 129: "L = 129"}.get(L, "L < 32" if L < 32 else None)
    live = ((L - 1) % 128) // 32 + 1
    return ("L", special, blocks_class(L), live, "ragged" if L % 32 else "whole")


def grid_key(S, L):
    wg = S * ((L + 31) // 32)
    return ("grid", "S = 1" if S == 1 else "S > 1", "< 8" if wg < 8 else "% 8 = 0" if wg % 8 == 0 else "% 8 != 0")


MIN_L = 33       # below it only the L key counts: with one sub-block (L = 1: one key, p = 1) the scores barely decide anything
MIN_C = 32       # below it only the channel and vec keys count: a score matrix of small rank puts every row's maximum on a
                 # handful of keys (C = 1: on two), and the key cond_ref.attn_input plants in the last block for row 5
                 # scores 1.07 sqrt(C) against a largest random score of about 3.5 -- from one full channel tile on (6.0) the
                 # running maximum of that row rises in the last block, below it need not


def keys(S, C, L, aq=0, ad=0):
    """The keys a shape earns.  The channel, vec, blocks and grid keys are earned only from L = 33 on (two sub-blocks, so
    that a wrong score, a wrong V run or a wrong view changes the output), the L, blocks and grid keys only from C = 32 on."""
    nt = tiles_per_wave(C)
    out = [chan_key(C), ("vec", nt, vec_state(aq, ad, L))] if L >= MIN_L else []
    if C >= MIN_C:
        out += [l_key(L)] + ([("blocks", nt, blocks_class(L)), grid_key(S, L)] if L >= MIN_L else [])
    return out


# ------------------------------------------------------------------------------------------------ the case list
Case = collections.namedtuple("Case", "S C L aq ad why")      # aq, ad: byte offsets of qkv and dO from a 16-byte boundary
DOMAIN_S = (1, 2, 3, 5, 8, 9)
DOMAIN_L = tuple(range(1, 521))
ALIGN = ((0, 0), (4, 0), (0, 4), (4, 4))


def c_id(c):
    return f"S{c.S}-C{c.C}-L{c.L}" + ("" if not (c.aq or c.ad) else f"-qkv+{c.aq}-dO+{c.ad}")


def cost(S, C, L):
    return S * L * L * C


def domain_C():
    """The smallest C of every channel class (the cost grows with C)."""
    first = {}
    for C in range(1, 513):
        first.setdefault(chan_key(C), C)
    return sorted(set(first.values()) | {MIN_C})


@functools.lru_cache(None)
def _enumerate():
    """-> (cases, covered keys, {key over the cap: its cheapest shape})."""
    dom = []
    for C in domain_C():
        for L in DOMAIN_L:
            for S in DOMAIN_S:
                for aq, ad in ALIGN if L % 4 == 0 else ALIGN[:1]:          # (with L % 4 != 0 the alignment decides nothing)
                    if not (aq and ad):                                     # (both misaligned: the plan of qkv misaligned)
                        dom.append((cost(S, C, L), S, C, L, aq, ad))
    dom.sort()
    cases, covered, over = [], set(), {}
    for cst, S, C, L, aq, ad in dom:
        new = [k for k in keys(S, C, L, aq, ad) if k not in covered]
        if not new:
            continue
        if cst > ATTN_CAP:
            for k in new:
                over.setdefault(k, (S, C, L, aq, ad))
            continue
        covered.update(new)
        cases.append(Case(S, C, L, aq, ad, "; ".join(" ".join(str(v) for v in k if v is not None) for k in new)))
    return tuple(cases), frozenset(covered), {k: v for k, v in over.items() if k not in covered}


def cases():
    return list(_enumerate()[0])


def covered():
    return set(_enumerate()[1])


def over_cap_classes():
    return dict(_enumerate()[2])


def all_keys():
    """Every key of the domain C = 1 .. 512, L = 1 .. 520, S in DOMAIN_S and the alignment states."""
    out = set()
    for C in range(1, 513):
        out.add(chan_key(C))
    for nt in range(1, 5):
        out |= {("vec", nt, s) for s in VEC_STATES} | {("blocks", nt, b) for b in ("1", "2", "3", ">= 4")}
    out |= {l_key(L) for L in DOMAIN_L} | {grid_key(S, L) for S in DOMAIN_S for L in DOMAIN_L}
    return out


MODEL_C = (32, 64, 192, 320)          # the envelope model's attention widths; SMALL and TINY: 64, 192, 320


def model_classes():
    """{key: first (S, C, L)} of every class a streaming attention of the models reaches at any L > 4096 (the classes are
    periodic in L with period 128 and in S x ceil(L / 32) with period 8: S = 1 .. 17 and 512 values of L reach them all)."""
    from attn_plan_ref import model_attention_shapes
    reached = {}
    for C in sorted(set(MODEL_C) | {c for c, _ in model_attention_shapes()[0]}):
        for L in range(4097, 4097 + 512):
            for S in range(1, 18):
                for k in keys(S, C, L):
                    reached.setdefault(k, (S, C, L))
    return reached


# ------------------------------------------------------------------------------------------------ inputs, references
def tensors(c):
    """-> (qkv (S, 3C, L), dO (S, C, L)) float32: cond_ref.attn_input at scale 2, shift 0 (every view different, the
    largest key of rows 5 and L / 2 in the last key block) wherever L allows it, plain uniform +-2 below L = 10."""
    if c.L >= 10:
        qkv = cr.attn_input(c.S, c.C, c.L, 2, 0, SEED)
    else:
        qkv = (2 * cr._u((c.S, 3 * c.C, c.L), SEED)).float()
    return qkv, cr._u((c.S, c.C, c.L), SEED + 7).float()


def rowstat_ref(qkv, dt):
    """(c2 max, 1 / sum) of every query row, c2 = log2 e / sqrt(C), in dtype dt with stock torch -> (S, 2, L)."""
    S, C3, L = qkv.shape
    C = C3 // 3
    q, k, _ = qkv.to(dt).reshape(S, 3, C, L).unbind(1)
    s = torch.bmm(q.transpose(1, 2), k) / math.sqrt(C)
    m = s.max(-1).values
    return torch.stack([m * LOG2E, 1.0 / torch.exp(s - m[:, :, None]).sum(-1)], 1)


@functools.lru_cache(None)
def refs(c):
    """-> (qkv, dO, r64, r32), each reference [out, dqkv, c2 max (S, L), 1 / sum (S, L)]; computed once per case."""
    qkv, dO = tensors(c)
    r64, r32 = cr.attn_ref(qkv, dO)
    s64, s32 = rowstat_ref(qkv, torch.float64), rowstat_ref(qkv, torch.float32)
    return qkv, dO, [r64[0], r64[1], s64[:, 0], s64[:, 1]], [r32[0].detach(), r32[1], s32[:, 0], s32[:, 1]]


def backward_ref_on_rounded(c):
    """The backward alone: out and rowstat made in float64 and rounded once to fp32, and the float64 / stock-order fp32
    d(qkv) of the backward fed exactly those -> (out32, rowstat32, d64, d32)."""
    qkv, dO, r64, _ = refs(c)
    out32, stat32 = r64[0].float(), torch.stack([r64[2], r64[3]], 1).float()
    d64 = model_backward(qkv, out32, dO, stat32)
    S, C3, L = qkv.shape
    C = C3 // 3
    q, k, v = qkv.reshape(S, 3, C, L).unbind(1)
    a = 1.0 / math.sqrt(C)
    p = torch.exp2(torch.bmm(q.transpose(1, 2), k) * (a * LOG2E) - stat32[:, 0, :, None]) * stat32[:, 1, :, None]
    ds = p * (torch.bmm(dO.transpose(1, 2), v) - (dO * out32).sum(1)[:, :, None])
    d32 = torch.stack([a * torch.bmm(k, ds.transpose(1, 2)), a * torch.bmm(q, ds), torch.bmm(dO, p)], 1).reshape(S, C3, L)
    return out32, stat32, d64, d32
