"""Channel level and power squelch on the device where tests/test_gpu_levels.py cannot see: under a DC offset, at the tile counts and tail
shapes that take the finish kernel's loop and the tail masks through every path, at stream counts that leave a workgroup of the finish kernel
partly idle, with both tile paths inside one block, and squelch at its edges (csrc/k_common.inc tile_level_sums / wave_sum_lane63, the LV
stores of csrc/kernel.inc, csrc/levels.inc).

The level rule here is rule B (levels_model.assert_rule_b): the device's level of a block equals levels_model.level_standin - the documented
summation order, step by step - of that launch's own `y` debug tap as float32, or is one ulp away (the one place the compiler has a choice: a
double fma in S2 / n - m1^2).  The tolerance of tests/test_gpu_levels.py is relative to the mean square; under a DC offset the mean square is
up to 10^6 times the variance the level is the root of, and that rule then accepts a level wrong by a factor of two
(tests/test_levels_cpu.py).  For the exact family, whose y is the oracle's bit for bit, the same comparison is made with the oracle's y.

Every level test prints (lvl - ref) / ref against float64 (levels_model.block_level of the tap) and the worst so far per input kind."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from levels_model import assert_rule_b, block_level, dc_bytes, level_standin, squelch_model  # noqa: E402
from test_gpu_levels import MATHS, NB, PATTERN, iq_of, math_of, squelch_input  # noqa: E402

pytestmark = pytest.mark.gpu

BL = 262144
STEREO = dict(rate_in=300000, rate_out2=48000, mode=2)
MONO = dict(rate_in=300000, rate_out2=48000, mode=1)
NFM = dict(rate_in=25000, rate_out2=12500, mode=1)
KWS = {"stereo_300k": STEREO, "mono_300k": MONO, "nfm_25k": NFM}
FAST3 = ["valu", "mfma", "mfma_f"]
WORST = {}                     # input kind -> largest |lvl - ref| / ref against float64 so far


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def bytes_of(spec, n_bytes):
    """read-only u8 [n_bytes] of an input spec: "lcg" / "dds" / "quiet" (tests/test_gpu_levels.py), ("dc", offset, kind, seed), or
    ("halves", first, second, block_len): blocks whose first half is one spec and whose second half is the other"""
    if isinstance(spec, str):
        a = np.array(iq_of(spec, n_bytes))
    elif spec[0] == "dc":
        a = dc_bytes(n_bytes, spec[1], spec[2], spec[3])
    elif spec[0] == "halves":
        bl = spec[3]
        a = np.array(bytes_of(spec[1], n_bytes)).reshape(-1, bl)
        a[:, bl // 2:] = bytes_of(spec[2], n_bytes).reshape(-1, bl)[:, bl // 2:]
        a = a.reshape(-1)
    else:
        raise ValueError(spec)
    a.setflags(write=False)
    return a


def kind_of(spec):
    return spec if isinstance(spec, str) else "dc %d %s" % spec[1:3] if spec[0] == "dc" else "%s | %s" % (kind_of(spec[1]), kind_of(spec[2]))


def capture(specs, nb, block_len):
    return np.stack([bytes_of(sp, nb * block_len) for sp in specs]).reshape(len(specs), nb, block_len)


@functools.lru_cache(maxsize=None)
def oracle_standin(kw_items, spec, block_len, nb):
    """level_standin of the oracle's y, block by block"""
    from oracle import OracleStream
    s = OracleStream(**dict(kw_items))
    iq = bytes_of(spec, nb * block_len)
    return [level_standin(s.block(iq[k * block_len:(k + 1) * block_len], trace=True)[1]["y"]) for k in range(nb)]


def launch(b, iq_np, levels=True, taps=False, pcm_fill=0, guard=64):
    """One run_device_levels launch of b over iq_np [S, nb, block_len].  dict: pcm [S, nb, stride], lens [S, nb], lv [S, nb] (or None),
    lv_guard (the `guard` entries behind the level buffer, prefilled with -1 like the buffer), y [S, nb, 2 M] (or None)."""
    import torch
    dev = torch.device("cuda:0")
    S, nb = iq_np.shape[:2]
    assert S == b.n_streams and iq_np.shape[2] == b.cfg.block_len
    M = b.cfg.block_len // 16
    iq = torch.from_numpy(np.ascontiguousarray(iq_np).reshape(-1)).to(dev)
    pcm = torch.full((S * nb * b.pcm_stride,), pcm_fill, dtype=torch.int16, device=dev)
    lens = torch.full((S * nb,), -7, dtype=torch.int32, device=dev)
    lv = torch.full((S * nb + guard,), -1.0, dtype=torch.float32, device=dev) if levels else None
    y = torch.zeros(S * nb * 2 * M, dtype=torch.float32, device=dev) if taps else None
    torch.cuda.synchronize()
    b.run_device_levels(iq, nb, pcm, lens, lv, debug={"y": y} if taps else None)
    b.sync()
    lvh = lv.cpu().numpy() if levels else None
    return {"pcm": pcm.cpu().numpy().reshape(S, nb, -1), "lens": lens.cpu().numpy().reshape(S, nb),
            "lv": lvh[:S * nb].reshape(S, nb) if levels else None, "lv_guard": lvh[S * nb:] if levels else None,
            "y": y.cpu().numpy().reshape(S, nb, 2 * M) if taps else None}


def check_rule_b(R, kw, math, specs, nb, block_len, split=0, want_bits=None):
    """One batch of len(specs) streams, one launch with the y tap (the DBG, LV build): every level written; rule B against the tap, and for
    the exact family against the oracle's y.  Returns the levels [S, nb]."""
    iq = capture(specs, nb, block_len)
    b = R.BatchDemod(R.wbfm_config(block_len=block_len, math=math_of(R, math), **kw), len(specs))
    b.set_time_split(split)
    r = launch(b, iq, taps=True)
    b.close()
    lv = r["lv"]
    assert (r["lv_guard"] == -1.0).all() and np.isfinite(lv).all() and (lv >= 0).all(), (lv, r["lv_guard"])
    for s, sp in enumerate(specs):
        what = "%s %s block_len %d stream %d (%s)" % (math, sorted(kw.items()), block_len, s, kind_of(sp))
        for k in range(nb):
            ref = block_level(r["y"][s, k])[0]
            rel = (float(lv[s, k]) - ref) / ref if ref > 0 else 0.0
            WORST[kind_of(sp)] = max(WORST.get(kind_of(sp), 0.0), abs(rel))
            print("%s block %d: level %.9g, float64 of the tap %.9g, relative error %+.2e" % (what, k, lv[s, k], ref, rel))
        assert_rule_b(lv[s], [level_standin(r["y"][s, k]) for k in range(nb)], what + ", own y tap")
        if math == "exact":
            assert_rule_b(lv[s], oracle_standin(tuple(sorted(kw.items())), sp, block_len, nb), what + ", the oracle's y")
    print("worst |lvl - ref| / ref against float64 so far, per input kind: %s" % ", ".join("%s %.1e" % kv for kv in sorted(WORST.items())))
    return lv


# ---- DC offset -----------------------------------------------------------------------------------------------------------------------------

DC_SPECS = [("dc", 12, "lsb", 1), ("dc", 12, "sig", 1), ("dc", 120, "lsb", 1), ("dc", 120, "sig", 1)]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "mono_300k"])
def test_level_under_a_dc_offset(R, name, math):
    """Offset tuning (no fs/4 rotation): the offset stays at DC in y and S2 / n - m1^2 cancels up to six digits.  Four streams - 12 and 120
    counts, one LSB of noise and 3 counts rms - two blocks: rule B; the build without taps gives the same bits."""
    kw = dict(KWS[name], offset_tuning=True)
    lv = check_rule_b(R, kw, math, DC_SPECS, 2, BL)
    b = R.BatchDemod(R.wbfm_config(block_len=BL, math=math_of(R, math), **kw), len(DC_SPECS))
    plain = launch(b, capture(DC_SPECS, 2, BL))["lv"]
    b.close()
    assert same_bits(plain, lv), (plain, lv)


@pytest.mark.parametrize("math", MATHS)
def test_level_under_a_dc_offset_with_the_rotation_on(R, math):
    """Without offset tuning the fs/4 rotation moves the offset to fs/4, where the decimator removes it: the level under 120 counts of offset
    is that of the noise (here: below twice the level of the same kind of noise without offset).  Rule B as everywhere."""
    specs = DC_SPECS[2:] + [("dc", 0, "lsb", 1), ("dc", 0, "sig", 1)]
    lv = check_rule_b(R, STEREO, math, specs, 2, BL)
    assert (lv[0] < 2 * lv[2]).all() and (lv[1] < 2 * lv[3]).all() and (lv[2] < 2 * lv[0]).all() and (lv[3] < 2 * lv[1]).all(), lv


# ---- tile counts and tail shapes -------------------------------------------------------------------------------------------------------------

SHAPES = [64, 80, 8192, 8208, 524288, 524368, 1048624]
"""block_len    M  tiles
        64      4      1   one half-filled lane
        80      5      1   half-filled lane, odd M
      8192    512      1   one full tile
      8208    513      2   the second tile holds one output
    524288  32768     64   exactly 64 tiles: one trip of the finish loop, every lane busy
    524368  32773     65   the 65th tile holds 5 outputs; a second trip for lane 0 alone
   1048624  65539    129   a third trip"""
SHAPE_SPECS = ["lcg", ("dc", 60, "lsb", 3)]


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "nfm_25k"])
@pytest.mark.parametrize("block_len", SHAPES)
def test_tile_counts_and_tail_shapes(R, block_len, name, math):
    check_rule_b(R, dict(KWS[name], offset_tuning=True), math, SHAPE_SPECS, 2, block_len)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "nfm_25k"])
def test_65_tiles_do_not_depend_on_time_split_or_launch_split(R, name, math):
    block_len, nb = 524368, 2
    iq = capture(SHAPE_SPECS, nb, block_len)
    cfg = R.wbfm_config(block_len=block_len, math=math_of(R, math), offset_tuning=True, **KWS[name])
    got = {}
    for split in (0, 48):
        b = R.BatchDemod(cfg, 2)
        b.set_time_split(split)
        got[split] = b.run_host_levels(iq, nb)[2]
        b.close()
    b = R.BatchDemod(cfg, 2)
    got["1+1"] = np.concatenate([b.run_host_levels(np.ascontiguousarray(iq[:, k:k + 1]), 1)[2] for k in range(nb)], axis=1)
    b.close()
    bad = {k: v for k, v in got.items() if not same_bits(v, got[0])}
    assert not bad, "levels differ from the default launch's %s: %s" % (got[0], bad)


# ---- stream counts ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("n_streams", [2, 3, 5])
def test_stream_counts_that_leave_a_workgroup_partly_idle(R, n_streams, math):
    """The finish kernel runs four streams per workgroup: 2 and 3 leave waves of the only workgroup idle, 5 puts one stream into a second.
    Every stream has its own input (the last one quiet).  Rule B per stream; exactly S x B levels are written (the buffer and 64 entries
    behind it are prefilled with -1); a stream's levels are the bits it gives alone."""
    nb, block_len = 3, 40000                                # M = 2500: four tiles and 452 outputs, the last lane with four
    specs = [("dc", (12, 120, 60, 36)[k], ("lsb", "sig")[k & 1], 10 + k) for k in range(n_streams - 1)] + ["quiet"]
    kw = dict(STEREO, offset_tuning=True)
    lv = check_rule_b(R, kw, math, specs, nb, block_len)     # (asserts every entry written and the guard untouched)
    for s, sp in enumerate(specs):
        b = R.BatchDemod(R.wbfm_config(block_len=block_len, math=math_of(R, math), **kw), 1)
        alone = launch(b, capture([sp], nb, block_len))["lv"]
        b.close()
        assert same_bits(alone[0], lv[s]), (s, alone[0], lv[s])


# ---- both tile paths inside one block ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", FAST3)
@pytest.mark.parametrize("offset_tuning", [False, True])
def test_both_tile_paths_inside_one_block(R, offset_tuning, math):
    """Blocks whose first half is one LSB of noise - the fast kernels' exact-tile path and its predicted successors, whose sums are the re-sum
    after exact_tile_decimate - and whose second half is a loud FM signal - the fast path's first sum; and the reverse.  One level takes
    partials from both."""
    specs = [("halves", "quiet", "dds", BL), ("halves", "dds", "quiet", BL)]
    check_rule_b(R, dict(STEREO, offset_tuning=offset_tuning), math, specs, 2, BL)


# ---- squelch edges -----------------------------------------------------------------------------------------------------------------------------

def sq_math(R, math):
    return R.MATH_EXACT if math == "exact" else R.MATH_FAST


def run_parts(b, iq, parts, path):
    """iq [S, sum(parts), BL] in launches of parts[i] blocks: (pcm, lens, levels or None); path "host_levels", or "device" = run_device_levels
    without a level buffer (squelch alone)"""
    out, k0 = [], 0
    for per in parts:
        x = np.ascontiguousarray(iq[:, k0:k0 + per])
        if path == "host_levels":
            out.append(b.run_host_levels(x, per))
        else:
            r = launch(b, x, levels=False)
            out.append((r["pcm"], r["lens"], None))
        k0 += per
    lv = None if out[0][2] is None else np.concatenate([o[2] for o in out], axis=1)
    return np.concatenate([o[0] for o in out], axis=1), np.concatenate([o[1] for o in out], axis=1), lv


_UNSQ = {}


def unsquelched(R, math, parts=(NB,), rows=(0, 1, 2, 3)):
    """(pcm, lens, levels) of squelch_input()'s streams `rows` without squelch, in launches of `parts` blocks (shared, read-only)"""
    key = (math, tuple(parts), tuple(rows))
    if key not in _UNSQ:
        b = R.BatchDemod(R.wbfm_config(math=sq_math(R, math), **STEREO), len(rows))
        res = run_parts(b, squelch_input()[list(rows)], parts, "host_levels")
        b.close()
        for a in res:
            a.setflags(write=False)
        assert (res[1] > 0).all()
        _UNSQ[key] = res
    return _UNSQ[key]


def between(lv0, rows=(0, 1, 2, 3)):
    """a threshold between the quiet and the loud blocks of squelch_input()"""
    pats = [PATTERN[s:] + PATTERN[:s] for s in rows]
    loud = [lv0[i, k] for i in range(len(rows)) for k in range(NB) if pats[i][k] == "L"]
    quiet = [lv0[i, k] for i in range(len(rows)) for k in range(NB) if pats[i][k] == "Q"]
    t = float(np.sqrt(max(quiet) * min(loud)))
    assert max(quiet) < t < min(loud), (quiet, loud)
    return t


def closed_set(pcm, lens, p0, l0):
    """[S, B] bool: which slots are closed (lens 0, the whole stride zero); every other slot must be the unsquelched run's"""
    S, B = lens.shape
    closed = np.zeros((S, B), bool)
    for s in range(S):
        for k in range(B):
            if lens[s, k] == 0 and not pcm[s, k].any():
                closed[s, k] = True
            else:
                assert lens[s, k] == l0[s, k] and np.array_equal(pcm[s, k, :lens[s, k]], p0[s, k, :l0[s, k]]), (s, k, lens[s, k], l0[s, k])
    return closed


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_threshold_equal_to_a_level(R, math):
    """`level < thr` is strict: a stream whose threshold IS the level of block k keeps that block open; its twin, with the next float32 above
    as threshold, closes it (conseq 0, so each block decides for itself)."""
    rows, k = (1, 1), 2                                     # stream 1 of squelch_input() twice: Q Q Q L Q L Q L
    p0, l0, lv0 = unsquelched(R, math, rows=rows)
    assert same_bits(lv0[0], lv0[1])
    t = np.float32(lv0[0, k])
    thr = np.array([t, np.nextafter(t, np.float32(np.inf))], np.float32)
    want, want_hits = squelch_model(lv0, thr, 0)
    assert not want[0, k] and want[1, k] and want[1].sum() == want[0].sum() + 1
    b = R.BatchDemod(R.wbfm_config(math=sq_math(R, math), **STEREO), 2)
    b.set_squelch(thr, 0)
    pcm, lens, lv = run_parts(b, squelch_input()[list(rows)], (NB,), "host_levels")
    hits = [b.squelch_hits(s) for s in range(2)]
    b.close()
    assert same_bits(lv, lv0)
    got = closed_set(pcm, lens, p0, l0)
    assert np.array_equal(got, want), (got, want)
    assert hits == want_hits


@pytest.mark.parametrize("path", ["host_levels", "device"])
@pytest.mark.parametrize("conseq", [0, 2])
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_one_block_launches_and_uneven_splits(R, math, conseq, path):
    """Eight one-block launches and 3 + 5: the hits carried from launch to launch close the blocks, and leave the counters, of one launch of
    eight; open blocks are the unsquelched run's of the same split."""
    iq = squelch_input()
    _, _, lv0 = unsquelched(R, math)
    t = between(lv0)
    thr = np.array([0.0, t, 1e3, t], np.float32)
    want, want_hits = squelch_model(lv0, thr, conseq)
    assert want[1].any() and not want[1].all()
    res = {}
    for parts in ((NB,), (1,) * NB, (3, 5)):
        p0, l0, lvp = unsquelched(R, math, parts)
        assert same_bits(lvp, lv0)
        b = R.BatchDemod(R.wbfm_config(math=sq_math(R, math), **STEREO), 4)
        b.set_squelch(thr, conseq)
        pcm, lens, lv = run_parts(b, iq, parts, path)
        res[parts] = (closed_set(pcm, lens, p0, l0), [b.squelch_hits(s) for s in range(4)])
        b.close()
        assert lv is None or same_bits(lv, lv0)
    single = res[(NB,)]
    assert np.array_equal(single[0], want) and single[1] == [conseq + 1 if thr[s] <= 0 else want_hits[s] for s in range(4)], (single, want)
    for parts, (closed, hits) in res.items():
        assert np.array_equal(closed, single[0]) and hits == single[1], (parts, closed, hits, single)


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_conseq_limits(R, math):
    """conseq = 20, more than the run's eight blocks: a stream stays closed up to its first loud block and never closes again.  conseq = 2^30,
    the largest: accepted, the counters read 2^30 + 1 and a launch runs the recurrence on them."""
    iq = squelch_input()
    p0, l0, lv0 = unsquelched(R, math)
    t = between(lv0)
    thr = np.full(4, t, np.float32)
    for conseq in (20, 2 ** 30):
        want, want_hits = squelch_model(lv0, thr, conseq)
        for s in range(4):
            first_loud = (PATTERN[s:] + PATTERN[:s]).index("L")
            assert want[s].tolist() == [k < first_loud for k in range(NB)]
        b = R.BatchDemod(R.wbfm_config(math=sq_math(R, math), **STEREO), 4)
        b.set_squelch(thr, conseq)
        assert [b.squelch_hits(s) for s in range(4)] == [conseq + 1] * 4
        pcm, lens, lv = run_parts(b, iq, (NB,), "host_levels")
        hits = [b.squelch_hits(s) for s in range(4)]
        b.close()
        assert np.array_equal(closed_set(pcm, lens, p0, l0), want) and hits == want_hits and same_bits(lv, lv0), (conseq, hits, want_hits)


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_hits_set_between_launches_and_squelch_off_and_on_again(R, math):
    """4 + 4 blocks, conseq 2.  (a) fmd_batch_set_squelch_hits between the launches: the second launch continues from the counters as set.
    (b) squelch switched off between the launches: the second closes nothing; switched on again: every counter reads conseq + 1."""
    iq = squelch_input()
    conseq, parts = 2, (4, 4)
    p0, l0, lv0 = unsquelched(R, math, parts)
    t = between(lv0)
    thr = np.array([t, t, 1e3, t], np.float32)
    cfg = R.wbfm_config(math=sq_math(R, math), **STEREO)

    b = R.BatchDemod(cfg, 4)
    b.set_squelch(thr, conseq)
    first = run_parts(b, iq[:, :4], (4,), "host_levels")
    want1, hits1 = squelch_model(lv0[:, :4], thr, conseq)
    assert [b.squelch_hits(s) for s in range(4)] == hits1
    b.set_squelch_hits(1, 0)
    b.set_squelch_hits(2, 0)                                # (stream 2 is below its threshold throughout: it now stays open for two blocks)
    b.set_squelch_hits(3, conseq + 1)
    hits0 = [hits1[0], 0, 0, conseq + 1]
    assert [b.squelch_hits(s) for s in range(4)] == hits0
    second = run_parts(b, iq[:, 4:], (4,), "host_levels")
    want2, hits2 = squelch_model(lv0[:, 4:], thr, conseq, hits0=hits0)
    assert want2[2].tolist() == [False, False, True, True]
    assert not np.array_equal(want2, squelch_model(lv0[:, 4:], thr, conseq, hits0=hits1)[0])    # the set counters matter
    assert [b.squelch_hits(s) for s in range(4)] == hits2
    b.close()
    assert np.array_equal(closed_set(first[0], first[1], p0[:, :4], l0[:, :4]), want1)
    assert np.array_equal(closed_set(second[0], second[1], p0[:, 4:], l0[:, 4:]), want2)
    assert same_bits(np.concatenate([first[2], second[2]], axis=1), lv0)

    b = R.BatchDemod(cfg, 4)
    b.set_squelch(thr, conseq)
    first = run_parts(b, iq[:, :4], (4,), "host_levels")
    assert np.array_equal(closed_set(first[0], first[1], p0[:, :4], l0[:, :4]), want1) and want1.any()
    b.set_squelch(None)
    second = run_parts(b, iq[:, 4:], (4,), "device")         # no level buffer and no squelch: a plain launch
    assert not closed_set(second[0], second[1], p0[:, 4:], l0[:, 4:]).any()
    b.set_squelch(thr, conseq)
    assert [b.squelch_hits(s) for s in range(4)] == [conseq + 1] * 4
    b.close()


def small_block_input(block_len):
    """u8 [3, NB, block_len]: loud (dds) and quiet blocks in squelch_input()'s pattern"""
    loud, quiet = bytes_of("dds", NB * block_len).reshape(NB, block_len), bytes_of("quiet", NB * block_len).reshape(NB, block_len)
    return np.stack([np.stack([loud[k] if (PATTERN[s:] + PATTERN[:s])[k] == "L" else quiet[k] for k in range(NB)]) for s in range(3)])


@pytest.mark.parametrize("block_len", [BL, 80])
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_zeroes_the_whole_slot_and_nothing_else(R, math, block_len):
    """The device path with PCM prefilled with 0x5A5A, three streams: squelch off for stream 0 (threshold <= 0), stream 1 closed throughout
    between two streams with open blocks, stream 2 mixed.  A closed slot is zero over all pcm_stride values - at block_len 80 the stride is
    one 16-byte store, far fewer than the wave's 64 lanes - and every other slot, the prefill behind its length included, is the unsquelched
    run's."""
    iq = squelch_input()[:3] if block_len == BL else small_block_input(block_len)
    cfg = R.wbfm_config(block_len=block_len, math=sq_math(R, math), **STEREO)
    b = R.BatchDemod(cfg, 3)
    stride = b.pcm_stride
    u = launch(b, iq, pcm_fill=0x5A5A)
    b.close()
    assert stride % 8 == 0 and (block_len == BL or stride // 8 < 64) and u["pcm"].shape == (3, NB, stride)
    order = np.sort(u["lv"][2])
    assert order[2] < order[3]
    thr = np.array([-1.0, 1e3, order[3]], np.float32)         # stream 2: its three quietest blocks are below
    want, want_hits = squelch_model(u["lv"], thr, 0)
    assert not want[0].any() and want[1].all() and want[2].sum() == 3
    b = R.BatchDemod(cfg, 3)
    b.set_squelch(thr, 0)
    r = launch(b, iq, pcm_fill=0x5A5A)
    hits = [b.squelch_hits(s) for s in range(3)]
    b.close()
    assert same_bits(r["lv"], u["lv"]) and hits == [1] + want_hits[1:]
    for s in range(3):
        for k in range(NB):
            if want[s, k]:
                assert r["lens"][s, k] == 0 and not r["pcm"][s, k].any(), (s, k)
            else:
                assert r["lens"][s, k] == u["lens"][s, k] and np.array_equal(r["pcm"][s, k], u["pcm"][s, k]), (s, k)


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch_decides_on_the_dc_corrected_level(R, math):
    """120 counts of offset under offset tuning: the root mean square of y is ~0.9, its level (the offset removed) ~1e-3.  A threshold between
    the two closes the stream; a twin with a threshold below the level stays open."""
    nb = 2
    spec = ("dc", 120, "lsb", 1)
    iq = capture([spec, spec], nb, BL)
    cfg = R.wbfm_config(math=sq_math(R, math), offset_tuning=True, **STEREO)
    b = R.BatchDemod(cfg, 2)
    u = launch(b, iq, taps=True)
    b.close()
    rms = min(float(np.sqrt(block_level(u["y"][0, k])[1])) for k in range(nb))
    assert u["lv"].max() * 10 < rms, (u["lv"], rms)
    thr = np.array([np.sqrt(float(u["lv"].max()) * rms), float(u["lv"].min()) / 2], np.float32)
    want, want_hits = squelch_model(u["lv"], thr, 0)
    assert want[0].all() and not want[1].any()
    b = R.BatchDemod(cfg, 2)
    b.set_squelch(thr, 0)
    r = launch(b, iq)
    hits = [b.squelch_hits(s) for s in range(2)]
    b.close()
    assert same_bits(r["lv"], u["lv"]) and hits == want_hits
    assert np.array_equal(closed_set(r["pcm"], r["lens"], u["pcm"], u["lens"]), want)
