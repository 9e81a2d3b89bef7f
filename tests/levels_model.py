"""Python models of the batch API's channel level and power squelch (include/fmdemod_mi355x.h, "Channel level and power squelch"),
for tests/test_levels_cpu.py, tests/test_gpu_levels.py and tests/test_gpu_levels_edges.py."""
import numpy as np

TILE = 512                       # decimated outputs per tile of the fused kernel (TW, csrc/k_common.inc)
DC_OFFSETS = (0, 12, 60, 120)    # counts of DC offset on the bytes; 128 + 120 < 256: no byte of the "lsb" kind clips
DC_KINDS = ("lsb", "sig")
U32 = 2.0 ** -24                 # float32 unit roundoff


def block_level(y):
    """The reference's rms() (src/rtl_fm_player.c:737-755, step = 1) over one block's lowpassed buffer y (2 M interleaved I/Q floats), in
    float64 and without its integer truncation: sqrt(max(0, S2/n - (S1/n)^2))."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    s1, s2 = y.sum(), (y * y).sum()
    return float(np.sqrt(max(0.0, s2 / n - (s1 / n) ** 2))), s2 / n


def squelch_model(levels, thresholds, conseq, hits0=None):
    """rtl_fm's power squelch over levels [n_streams, n_blocks] (float32, as the library returns them): (closed [S, B] bool, final hits [S]).
    thresholds[s] <= 0: off for that stream (never closed, hits untouched).  hits0: the counters before the first block (default conseq + 1)."""
    levels = np.asarray(levels, dtype=np.float32)
    S, B = levels.shape
    hits = [conseq + 1] * S if hits0 is None else list(hits0)
    closed = np.zeros((S, B), dtype=bool)
    for s in range(S):
        t = np.float32(thresholds[s])
        if not t > 0:
            continue
        h = hits[s]
        for b in range(B):
            h = h + 1 if levels[s, b] < t else 0
            if h > conseq:
                h = conseq + 1
                closed[s, b] = True
        hits[s] = h
    return closed, hits


# ---- the device's arithmetic, step by step ----------------------------------------------------------------------------------------------

def _fma_sq(x, q):
    """fmaf(x, x, q) on float32 arrays: x * x is exact in float64 (48 bits); the sum is rounded to odd in float64 (TwoSum gives its error), so
    the one rounding to float32 that follows is the fma's single rounding (53 >= 24 + 2 bits: no double rounding)."""
    p = x.astype(np.float64) ** 2
    q = q.astype(np.float64)
    s = p + q
    bb = s - p
    e = (p - (s - bb)) + (q - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def tile_partials(y, tile=TILE, tail=None):
    """(t1, t2), float32 [tiles]: what lane 63 of the fused kernel's LV build stores per tile of one block's y (2 M interleaved floats) -
    tile_level_sums and wave_sum_lane63 (csrc/k_common.inc).  tail (altered stand-ins only): interleaved values left in the last tile's
    masked outputs instead of 0."""
    y = np.asarray(y, dtype=np.float32).reshape(-1, 2)
    M = y.shape[0]
    tiles = (M + tile - 1) // tile
    z = np.zeros((tiles * tile, 2), np.float32)
    z[:M] = y
    if tail is not None:
        t = np.asarray(tail, dtype=np.float32).reshape(-1, 2)[:tiles * tile - M]
        z[M:M + t.shape[0]] = t
    z = z.reshape(tiles, tile // 8, 8, 2)                   # [tile, lane, output of the lane, I / Q]
    a = np.zeros(z.shape[:2], np.float32)
    q = np.zeros(z.shape[:2], np.float32)
    for r in range(8):
        i, j = z[:, :, r, 0], z[:, :, r, 1]
        a = a + i
        a = a + j
        q = _fma_sq(i, q)
        q = _fma_sq(j, q)
    assert a.dtype == q.dtype == np.float32
    while a.shape[1] > 1:                                   # adjacent pairs, level by level
        a = a[:, 0::2] + a[:, 1::2]
        q = q[:, 0::2] + q[:, 1::2]
    return a[:, 0], q[:, 0]


def level_standin(y, tile=TILE, finish=np.float64, tail=None):
    """The float32 level of one block's y (2 M interleaved floats) in exactly the order DESIGN.md section 5a, csrc/k_common.inc and
    csrc/levels.inc state - what the device must return, not what it should approximate.

    Per tile of `tile` outputs (tile_level_sums): lane l owns outputs 8 l .. 8 l + 7, outputs at or beyond the tile's valid count count as 0;
    from a = q = 0 in float32, for each output in order  a += I; a += Q; q = fmaf(I, I, q); q = fmaf(Q, Q, q)  (every fma one rounding).  The
    64 lane values are then added in a pairwise tree of adjacent pairs, in float32.  Float addition commutes, so that tree IS the DPP order of
    wave_sum_lane63 as lane 63 sees it: quad_perm [1,0,3,2] adds lanes 2 k and 2 k + 1, quad_perm [2,3,0,1] adds the two pairs of a quad,
    row_half_mirror the two quads of a half row, row_mirror the two half rows, row_bcast:15 rows 0 + 1 and 2 + 3, row_bcast:31 the two halves
    of the wave - at every step both operands are complete sums of adjacent, equally long runs of lanes, whichever of the two the lane holds.

    Finish (fmd_levels_kernel), in float64: lane l sums the partials of tiles l, l + 64, ... in order, an xor butterfly with offsets 32 .. 1
    follows, then m1 = S1 / n, var = S2 / n - m1 m1 (n = 2 M), sqrt(max(var, 0)) rounded once to float32.

    finish, tail: for altered stand-ins (tests/test_levels_cpu.py) - the finish sums in another type, values left in the masked outputs."""
    n = np.asarray(y).size
    t1, t2 = tile_partials(y, tile, tail)
    tiles = t1.size
    trips = (tiles + 63) // 64
    pa = np.zeros(trips * 64, finish)
    pq = np.zeros(trips * 64, finish)
    pa[:tiles], pq[:tiles] = t1, t2
    pa, pq = pa.reshape(trips, 64), pq.reshape(trips, 64)
    a = np.zeros(64, finish)
    q = np.zeros(64, finish)
    for t in range(trips):                                  # (a lane without a tile in this trip adds nothing: + 0 is exact)
        a = a + pa[t]
        q = q + pq[t]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[lanes ^ o]
        q = q + q[lanes ^ o]
    nn = np.float64(n)
    m1 = np.float64(a[0]) / nn
    var = np.float64(q[0]) / nn - m1 * m1
    return np.float32(np.sqrt(var if var > 0.0 else 0.0))


def ulps_apart(a, b):
    """distance of two non-negative finite float32 values in units of the last place (0: the same bits)"""
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b) and a >= 0 and b >= 0, (a, b)
    return abs(int(a.view(np.uint32)) - int(b.view(np.uint32)))


def assert_rule_b(got, want, what=""):
    """Rule B: block by block the level equals the stand-in's as float32 or is one ulp away.  The one ulp has one cause: the compiler may or
    may not contract q / n - m1 * m1 into a double fma, which under cancellation can move the float32 result across one rounding boundary;
    every other step of the order is fixed.  No other tolerance."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = [(k, float(g), float(w), ulps_apart(g, w)) for k, (g, w) in enumerate(zip(got, want))
           if not (np.isfinite(g) and g >= 0) or ulps_apart(g, w) > 1]
    assert not bad, "%s: (block, level, stand-in, ulps apart): %s" % (what, bad)


def level_bound(y):
    """The largest |lvl^2 - ref^2| the arithmetic of level_standin allows on one block's y, ref = block_level(y)[0] (real arithmetic).

    Derivation, u = 2^-24, gamma_k = k u / (1 - k u), n = 2 M, S1 = sum y, S2 = sum y^2, m1 = S1 / n:
      * a tile's squares: a lane's 16 fmas round 16 times, the six levels of the wave's tree six more - a term sees at most 22 roundings, and
        every term is non-negative, so the computed tile sum is within gamma_22 of itself; the finish adds the tiles in double (at most
        tiles / 64 + 6 additions, 2^-53 each: the DBL term below, which also pays for the reference's own float64 sums):
          |S2' - S2| <= gamma_22 S2;
      * a tile's sums: the lane's first addition is to 0 and exact, 15 round, the tree six more - 21 roundings, signs mixed:
          |S1' - S1| <= gamma_21 sum |y|;
      * var' = S2' / n - (S1' / n)^2:  |var' - var| <= gamma_22 S2 / n + 2 |m1| gamma_21 mean|y| + (gamma_21 mean|y|)^2 =: d;
      * max(var', 0) is no further from var >= 0 than var' is; the square root in double and the one rounding to float32 give
        lvl = sqrt(max(var', 0)) (1 + e), |e| <= u (1 + 2^-28):  |lvl^2 - var| <= d + 2.001 u (var + d).
    bound = d + 2.001 u (var + d) + DBL (S2 / n + m1^2) + 2^-149.

    For the CPU test of the stand-in only.  Under a DC offset S2 / n is thousands of times the variance, so this worst case is WIDER than the
    variance there: it cannot hold the device to its level, which is why the GPU tests use assert_rule_b against the stand-in instead."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    g22, g21 = 22 * U32 / (1 - 22 * U32), 21 * U32 / (1 - 21 * U32)
    ms, m1, ma = (y * y).sum() / n, y.sum() / n, np.abs(y).sum() / n
    var = max(0.0, ms - m1 * m1)
    d = g22 * ms + 2 * abs(m1) * g21 * ma + (g21 * ma) ** 2
    dbl = (n // (2 * TILE * 64) + 64) * 2.0 ** -53
    return float(d + 2.001 * U32 * (var + d) + dbl * (ms + m1 * m1) + 2.0 ** -149)


def dc_bytes(n_bytes, offset, kind, seed=1):
    """u8 IQ whose mean sits `offset` counts above the ADC's midpoint 127.5 (a dongle in offset-tuning mode delivers a few counts):
    "lsb": bytes in {127 + offset, 128 + offset} (one LSB of noise); "sig": 127.5 + offset + Gaussian noise of 3 counts rms, rounded and
    clipped to 0 .. 255."""
    rng = np.random.default_rng([int(seed), int(offset), DC_KINDS.index(kind)])
    if kind == "lsb":
        assert 0 <= 127 + offset and 128 + offset <= 255, offset
        return (rng.integers(127, 129, n_bytes) + offset).astype(np.uint8)
    if kind == "sig":
        return np.clip(np.rint(127.5 + offset + 3.0 * rng.standard_normal(n_bytes)), 0, 255).astype(np.uint8)
    raise ValueError(kind)
