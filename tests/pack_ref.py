"""The five packed-weight formats restated from their documented shape (pad, reshape, transpose), their sizes, an unpack
per format, the two input kinds and the comparison rule of tests/test_pack_host.py and tests/test_gpu_pack.py.  Imports no
GPU code.

Formats (M = the 64-row tile dimension, K = the chunk dimension; forward M = Cout, K = Cin, backward M = Cin, K = Cout):

  direct   csrc/conv.hip:pack_one            [M tile][K chunk][group][m 64][k 8] fp32.  3x3: group = tap, chunk = 8
                                             channels; 1x1: group = 8-channel sub-chunk, chunk = 32 channels.  Backward:
                                             co and ci exchanged, taps reversed.  Zero padded to whole tiles / chunks.
  wino     csrc/winograd24.hip:wino_pack_group   [M tile][K chunk][slice 6 a + b][m 64][k 8] = G2 w G4^T, transformed row 3
                                             NEGATED; backward: of the 180-degree-rotated kernel.
  wino44   csrc/winograd44f.hip:f44_pack_group   [M tile][K chunk][p][m 64][k 8] = G4 w G4^T at p = F44_P[6 a + b].
  small    csrc/conv_small.hip:conv3_small_pack_kernel   [16-row block][wave 8][round][group 5][quarter 4][row 16][4]: row
                                             16 blk + j, wave wv, round r hold the products (channel, tap) of the wave's
                                             channels wv cw + 8 r ... + 8 (cw = Cin / 8 channels per wave), 72 consecutive
                                             floats of the OIHW row, as five groups of 16 (the last one half empty); zero
                                             past the round's products and past Cout.  2 ceil(Cout / 32) blocks.
  bf16x3   csrc/conv1x1_bf16x3.hip:conv1x1_bf16x3_pack_kernel   [M tile 128][K chunk 32][k-step 2][row block 4][plane 3]
                                             [lane 64 = (k half 2, row 32)][8 bf16]; planes = RNE bf16 of w, w - p1,
                                             w - p1 - p2 (exact in fp32).

The rule (judge):
  * direct, small, bf16x3: every data element bit-identical to the restatement;
  * wino / wino44 on lattice weights (w = 576 n 2^-16, |n| <= 32): every intermediate of both transforms is an integer
    times 2^-16 below 2^24, so ANY evaluation order in any precision gives the same bits: bit-identical to the exact
    integer result (a computed zero of either sign equals zero);
  * wino / wino44 on random weights: |got - r64| <= half_ulp32(r64) + 2^-45 max|taps of that (co, ci)|, r64 the float64
    einsum; the second term covers the ordering error of two double evaluations under cancellation.  (Bit equality with
    round(r64) is NOT asserted: about 0.7 % of the true values are exact fp32 ties, which two correct double evaluations
    round to different sides.)
  * padding compares equal to zero (either sign); any non-finite value fails; nothing is skipped or filtered.
The reported value is max (|got - r64| - slack) / half_ulp32(r64): <= 1 passes (0 for the bitwise formats when equal)."""
import numpy as np

TCO = 64                # rows per tile: direct and both Winograd packs
CK3, CK1 = 8, 32        # channels per chunk: 3x3 / Winograd, 1x1
WINO_SLICES = {1: 24, 2: 36}
B3_TCO, B3_KC = 128, 32

G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
               [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=np.float64)
G2_X2 = np.array([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], dtype=np.int64)                       # 2 G2
G4_X24 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=np.int64)   # 24 G4
NESTED_ROW_SIGN = np.array([1, 1, 1, -1], dtype=np.int64)

# F(4x4): slice (transformed row a, transformed column b) -> position in wave order (wave g owns one full row and half of
# the row it shares with its neighbour: rows 0 | 1 lo, 2 | 1 hi, 3 | 4 lo, 5 | 4 hi)
F44_P = np.array([0, 1, 2, 3, 4, 5,
                  6, 7, 8, 15, 16, 17,
                  9, 10, 11, 12, 13, 14,
                  18, 19, 20, 21, 22, 23,
                  24, 25, 26, 33, 34, 35,
                  27, 28, 29, 30, 31, 32], dtype=np.int64)

LATTICE_UNIT = 576.0 * 2.0 ** -16
SLACK = 2.0 ** -45


def rup(v, m):
    return -(-v // m) * m


# ------------------------------------------------------------------------------------------------ inputs
def lattice(Cout, Cin, KS, seed):
    """w = 576 n 2^-16, integer |n| <= 32: both Winograd transforms are exact on it in fp32 and in double."""
    n = np.random.default_rng(seed).integers(-32, 33, size=(Cout, Cin, KS, KS))
    return (n * LATTICE_UNIT).astype(np.float32)


def lattice_ints(w):
    n = np.rint(w.astype(np.float64) / LATTICE_UNIT).astype(np.int64)
    assert np.array_equal((n * LATTICE_UNIT).astype(np.float32), w) and np.abs(n).max() <= 32
    return n


def normal(Cout, Cin, KS, seed):
    return np.random.default_rng(seed).standard_normal((Cout, Cin, KS, KS), dtype=np.float32)


# ------------------------------------------------------------------------------------------------ sizes
def direct_sizes(Cout, Cin, KS):
    ck = CK3 if KS == 3 else CK1
    return KS * KS * rup(Cin, ck) * rup(Cout, TCO), KS * KS * rup(Cout, ck) * rup(Cin, TCO)


def wino_sizes(kind, Cout, Cin):
    ns = WINO_SLICES[kind]
    return ns * rup(Cin, CK3) * rup(Cout, TCO), ns * rup(Cout, CK3) * rup(Cin, TCO)


def small_floats(Cout, Cin):
    nr = -(-(Cin // 8) // 8)                    # rounds of 8 channels of a wave's Cin / 8
    return -(-Cout // 32) * 2 * 8 * nr * 5 * 64 * 4


def b3_dwords(M, K):
    return -(-M // B3_TCO) * -(-K // B3_KC) * 2 * 4 * 3 * 64 * 4


# ------------------------------------------------------------------------------------------------ the tile layout
def _oriented(w, bwd):
    """[M][K][kh][kw]: the OIHW tensor, or for a backward pack co and ci exchanged and the kernel rotated by 180 degrees."""
    return w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1] if bwd else w


def _tiles(a):
    """a [M][K chunk][group][8] -> flat [M tile][K chunk][group][m 64][k 8], M zero padded to whole tiles."""
    M, nch, G, _ = a.shape
    a = np.pad(a, ((0, rup(M, TCO) - M), (0, 0), (0, 0), (0, 0)))
    return np.ascontiguousarray(a.reshape(-1, TCO, nch, G, 8).transpose(0, 2, 3, 1, 4)).reshape(-1)


def _untiles(p, M, nch, G):
    a = np.asarray(p).reshape(rup(M, TCO) // TCO, nch, G, TCO, 8).transpose(0, 3, 1, 2, 4).reshape(-1, nch, G, 8)
    return a[:M]


def _chunks_3x3(v):
    """v [M][K][G] (G taps or slices) -> [M][K chunk][G][8], K zero padded to whole 8-channel chunks."""
    M, K, G = v.shape
    v = np.pad(v, ((0, 0), (0, rup(K, CK3) - K), (0, 0)))
    return v.reshape(M, -1, CK3, G).transpose(0, 1, 3, 2)


def _unchunks_3x3(a, K):
    M, nch, G, _ = a.shape
    return a.transpose(0, 1, 3, 2).reshape(M, nch * CK3, G)[:, :K]


# ------------------------------------------------------------------------------------------------ direct
def direct_pack(w, bwd=False):
    v = _oriented(w, bwd)
    M, K, KS, _ = v.shape
    if KS == 3:
        return _tiles(_chunks_3x3(v.reshape(M, K, 9)))
    v = np.pad(v.reshape(M, K), ((0, 0), (0, rup(K, CK1) - K)))
    return _tiles(v.reshape(M, -1, 4, 8))


def direct_unpack(p, Cout, Cin, KS, bwd=False):
    M, K = (Cin, Cout) if bwd else (Cout, Cin)
    if KS == 3:
        v = _unchunks_3x3(_untiles(p, M, rup(K, CK3) // CK3, 9), K).reshape(M, K, 3, 3)
    else:
        v = _untiles(p, M, rup(K, CK1) // CK1, 4).reshape(M, -1)[:, :K].reshape(M, K, 1, 1)
    return np.ascontiguousarray(_oriented(v, bwd))          # (the orientation is its own inverse)


# ------------------------------------------------------------------------------------------------ Winograd
def wino_values(w, kind, bwd=False, dtype=np.float64):
    """U [M][K][a][b] = G w G4^T (G = G2 with row 3 negated for the nested kernel, G4 for F(4x4)), one einsum in `dtype`."""
    v = np.ascontiguousarray(_oriented(w, bwd)).astype(dtype)
    rows = (G2 * NESTED_ROW_SIGN[:, None]) if kind == 1 else G4
    return np.einsum("ai,mkij,bj->mkab", rows.astype(dtype), v, G4.astype(dtype))


def wino_values_exact(w, kind, bwd=False):
    """The same on lattice weights, in integers: U = (2 G2) n (24 G4)^T 12 2^-16 resp. (24 G4) n (24 G4)^T 2^-16."""
    n = np.ascontiguousarray(_oriented(lattice_ints(w), bwd))
    if kind == 1:
        u = np.einsum("ai,mkij,bj->mkab", G2_X2 * NESTED_ROW_SIGN[:, None], n, G4_X24) * 12
    else:
        u = np.einsum("ai,mkij,bj->mkab", G4_X24, n, G4_X24)
    assert np.abs(u).max() < 2 ** 24
    return (u.astype(np.float64) * 2.0 ** -16).astype(np.float32)


def wino_values_kernel_order(w, kind, bwd=False, dtype=np.float64):
    """Another evaluation of the same transforms: the factored formulas of the pack kernels' comments (rows first, the
    column transform through the shared sums a6, b6, a24, b12), every operation in `dtype`."""
    g = np.ascontiguousarray(_oriented(w, bwd)).astype(dtype)
    c = lambda x: dtype(x)

    def g4(x0, x1, x2):
        a6, b6 = -(x0 + x2) / c(6), x1 / c(6)
        a24, b12 = x0 / c(24) + x2 / c(6), x1 / c(12)
        return [x0 / c(4), a6 - b6, a6 + b6, a24 + b12, a24 - b12, x2]

    if kind == 1:
        h, e = c(0.5) * (g[:, :, 0] + g[:, :, 2]), c(0.5) * g[:, :, 1]
        rows = [g[:, :, 0], h + e, h - e, -g[:, :, 2]]
    else:
        rows = g4(g[:, :, 0], g[:, :, 1], g[:, :, 2])
    return np.stack([np.stack(g4(r[..., 0], r[..., 1], r[..., 2]), -1) for r in rows], 2)


def wino_layout(u, kind):
    """u [M][K][a][b] -> the flat pack."""
    M, K = u.shape[:2]
    s = u.reshape(M, K, -1)
    if kind == 2:
        t = np.empty_like(s)
        t[:, :, F44_P] = s
        s = t
    return _tiles(_chunks_3x3(s))


def wino_pack(w, kind, bwd=False, dtype=np.float64):
    """The flat pack in `dtype` (float64: r64 of the rule)."""
    return wino_layout(wino_values(w, kind, bwd, dtype), kind)


def wino_pack_exact(w, kind, bwd=False):
    return wino_layout(wino_values_exact(w, kind, bwd), kind)


def wino_slices(p, kind, Cout, Cin, bwd=False):
    """The flat pack -> U [M][K][a][b]."""
    M, K = (Cin, Cout) if bwd else (Cout, Cin)
    ns = WINO_SLICES[kind]
    s = _unchunks_3x3(_untiles(p, M, rup(K, CK3) // CK3, ns), K)
    if kind == 2:
        s = s[:, :, F44_P]
    return s.reshape(M, K, ns // 6, 6)


def wino_unpack(p, kind, Cout, Cin, bwd=False):
    """OIHW (float64) from a Winograd pack.  Rows: g0 = U[0], g2 = U[last] (negated back for the nested kernel) and, nested,
    g1 = U[1] - U[2], F(4x4) g1 = 3 (U[2] - U[1]); columns: x0 = 4 c0, x1 = 3 (c2 - c1), x2 = c5.  The four corner taps come
    from one stored value each (times 4, 16, 1 or -1: exact for any weights); the others are exact on lattice weights."""
    u = wino_slices(p, kind, Cout, Cin, bwd).astype(np.float64)
    if kind == 1:
        r = np.stack([u[:, :, 0], u[:, :, 1] - u[:, :, 2], -u[:, :, 3]], 2)
    else:
        r = np.stack([4 * u[:, :, 0], 3 * (u[:, :, 2] - u[:, :, 1]), u[:, :, 5]], 2)
    v = np.stack([4 * r[..., 0], 3 * (r[..., 2] - r[..., 1]), r[..., 5]], -1)
    return np.ascontiguousarray(_oriented(v, bwd))


# ------------------------------------------------------------------------------------------------ small
def small_pack(w):
    Cout, Cin = w.shape[:2]
    cw = Cin // 8                              # channels per wave
    nr = -(-cw // 8)
    nblk = 2 * -(-Cout // 32)
    v = np.pad(w.reshape(Cout, 8, cw, 9), ((0, 16 * nblk - Cout), (0, 0), (0, 8 * nr - cw), (0, 0)))
    v = np.pad(v.reshape(nblk, 16, 8, nr, 72), ((0, 0),) * 4 + ((0, 8),))            # 72 products -> five groups of 16
    return np.ascontiguousarray(v.reshape(nblk, 16, 8, nr, 5, 4, 4).transpose(0, 2, 3, 4, 5, 1, 6)).reshape(-1)


def small_unpack(p, Cout, Cin):
    cw = Cin // 8
    nr = -(-cw // 8)
    nblk = 2 * -(-Cout // 32)
    v = np.asarray(p).reshape(nblk, 8, nr, 5, 4, 16, 4).transpose(0, 5, 1, 2, 3, 4, 6).reshape(nblk * 16, 8, nr, 80)[..., :72]
    return np.ascontiguousarray(v.reshape(nblk * 16, 8, nr * 8, 9)[:Cout, :, :cw].reshape(Cout, Cin, 3, 3))


# ------------------------------------------------------------------------------------------------ bf16x3
def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even, in integer arithmetic (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def b3_split(x):
    """-> three bf16 bit planes [3][...]; the fp32 differences are exact (each residual has fewer significant bits)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    p1 = bf16_rne(x)
    r1 = x - bf16_value(p1)
    p2 = bf16_rne(r1)
    r2 = r1 - bf16_value(p2)
    assert np.array_equal(r1.astype(np.float64), x.astype(np.float64) - bf16_value(p1).astype(np.float64))
    assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - bf16_value(p2).astype(np.float64))
    return np.stack([p1, p2, bf16_rne(r2)])


def b3_pack(w, bwd=False):
    """-> uint16 [2 dwords]: the low half of a dword is the even element."""
    v = w.reshape(w.shape[0], w.shape[1])
    v = v.T if bwd else v
    M, K = v.shape
    v = np.pad(v, ((0, rup(M, B3_TCO) - M), (0, rup(K, B3_KC) - K)))
    p = b3_split(v).reshape(3, -1, 4, 32, v.shape[1] // B3_KC, 2, 2, 8)      # [plane][tile][row block][row][chunk][k-step][k half][8]
    return np.ascontiguousarray(p.transpose(1, 4, 5, 2, 0, 6, 3, 7)).reshape(-1)


def b3_unpack(p, Cout, Cin, bwd=False):
    M, K = (Cin, Cout) if bwd else (Cout, Cin)
    nt, nch = rup(M, B3_TCO) // B3_TCO, rup(K, B3_KC) // B3_KC
    q = np.asarray(p).reshape(nt, nch, 2, 4, 3, 2, 32, 8).transpose(4, 0, 3, 6, 1, 2, 5, 7).reshape(3, nt * B3_TCO, nch * B3_KC)
    v = bf16_value(q).astype(np.float64).sum(0)[:M, :K].astype(np.float32)
    return np.ascontiguousarray((v.T if bwd else v).reshape(Cout, Cin, 1, 1))


# ------------------------------------------------------------------------------------------------ masks and the rule
def data_mask(fmt, Cout, Cin, bwd=False, KS=3):
    """1 where the pack holds a weight (or a value derived from one), 0 where it holds padding."""
    ones = np.ones((Cout, Cin, KS, KS), dtype=np.float32)
    if fmt == "direct":
        return direct_pack(ones, bwd) != 0
    if fmt in ("wino", "wino44"):
        kind = 1 if fmt == "wino" else 2
        return wino_layout(np.ones(_oriented(ones, bwd).shape[:2] + (WINO_SLICES[kind] // 6, 6)), kind) != 0
    if fmt == "small":
        return small_pack(ones) != 0
    assert fmt == "bf16x3"
    m = b3_pack(ones, bwd).reshape(-1, 3, 64 * 8)
    return np.broadcast_to(m[:, :1] != 0, m.shape).reshape(-1)          # (the residual planes of 1.0 are zero: data all the same)


def tap_max(w, kind, bwd=False):
    """max |tap| of each (co, ci), laid out like the pack: the scale of the rule's second term."""
    t = np.abs(_oriented(w, bwd)).astype(np.float64).max((2, 3))
    return wino_layout(np.broadcast_to(t[:, :, None, None], t.shape + (WINO_SLICES[kind] // 6, 6)), kind)


def half_ulp32(r):
    """Half the spacing of fp32 at |r| (r float64; the subnormal spacing below 2^-126)."""
    _, ex = np.frexp(np.abs(r))                       # |r| = m 2^ex, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(ex - 25, -150))


def judge_bits(got, want, mask, zero_sign=True):
    """The bitwise formats (and Winograd on lattice weights).  -> (passes, value, why); value 0.0 when equal.
    zero_sign=False (Winograd only): a computed zero may carry either sign -- -(x0 + x2) / 6 of two zeros is -0 where the
    integer result is +0 -- so a zero equals a zero; every other value is compared by its bits."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.shape != want.shape:
        return False, float("inf"), f"size {got.size} != {want.size}"
    if got.dtype == np.uint16:
        if (((got & 0x7F80) == 0x7F80)).any():
            return False, float("inf"), "non-finite value"
        bad_pad = ((got & 0x7FFF) != 0) & ~mask
    else:
        assert got.dtype == np.float32 and want.dtype == np.float32
        if not np.isfinite(got).all():
            return False, float("inf"), "non-finite value"
        bad_pad = (got != 0) & ~mask
        both_zero = (got == 0) & (want == 0)
        got, want = got.view(np.uint32), want.view(np.uint32)
        if not zero_sign:
            mask = mask & ~both_zero
    if bad_pad.any():
        return False, float("inf"), f"padding element {int(np.argmax(bad_pad))} is not zero"
    bad = (got != want) & mask
    if bad.any():
        return False, float("inf"), f"{int(bad.sum())} data elements differ, first at {int(np.argmax(bad))}"
    return True, 0.0, "bit-identical"


def judge_wino(got, r64, mask, slack_scale):
    """Winograd on arbitrary weights.  -> (passes, value, why), value = max (|got - r64| - slack) / half_ulp32(r64)."""
    got, r64 = np.asarray(got).reshape(-1), np.asarray(r64).reshape(-1)
    assert got.dtype == np.float32 and r64.dtype == np.float64
    if got.shape != r64.shape:
        return False, float("inf"), f"size {got.size} != {r64.size}"
    if not np.isfinite(got).all():
        return False, float("inf"), "non-finite value"
    bad_pad = (got != 0) & ~mask
    if bad_pad.any():
        return False, float("inf"), f"padding element {int(np.argmax(bad_pad))} is not zero"
    v = (np.abs(got.astype(np.float64) - r64) - SLACK * slack_scale.reshape(-1)) / half_ulp32(r64)
    worst = float(v[mask].max())
    n = int((v[mask] > 1.0).sum())
    return n == 0, worst, f"{n} of {int(mask.sum())} values beyond the bound"


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
EDGES = [(64, 6), (6, 64), (65, 9), (63, 7), (96, 40), (128, 64), (200, 96)]          # (Cout, Cin): the padding edges
EDGES_1X1 = EDGES + [(65, 33), (64, 32)]
# small: Cin a multiple of 32 (one half round, one full, two rounds with a half last one, two full), Cout around 16 and 32
SMALL_EDGES = [(co, ci) for ci in (32, 64, 96, 128) for co in (15, 16, 17, 31, 32, 33)]
# one grouped launch: a padded layer first and last, the smallest layer (one tile, one chunk per direction) between two
# multi-tile layers; eight layers, so the binary search takes both branches at each of its three depths
MULTI_3X3 = [(65, 9), (128, 64), (6, 6), (200, 96), (64, 8), (96, 40), (64, 6), (63, 7)]
MULTI_DIRECT = [(65, 9, 3), (128, 64, 3), (6, 6, 1), (200, 96, 1), (64, 32, 1), (96, 40, 3), (64, 6, 3), (63, 7, 1)]
