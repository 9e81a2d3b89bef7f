"""The device-free resolver (csrc/fmd_resolve.c) against an independent numpy model: the tap quantiser's integers, the decimating second stage's tap
tables byte for byte, the composite L+R taps, and that fmd_config_error_estimate speaks of the same quantised filters.

Everything is asked through the `t` query of tests/c/plan_check.c (the private fmdk_resolve / fmdk_dec_tables, linked from the library's objects) and
modelled from fmd_design_taps' float taps: a float tap times 2^qf is exact in double, so the model holds on any libm."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_launch_plan import plan_check  # noqa: E402,F401  (the fixture: builds tests/c/plan_check.c)
import rtl_fm_player_amd as R  # noqa: E402

T_MAX = 8355711                                    # the largest T three balanced int8 limbs hold
DG_N, K0G, DF_N, K0F, DM_N, K0M = 416, 180, 288, 92, 368, 128      # FMDK_DG_N .. FMDK_DEC_K0M (csrc/fmd_internal.h)

STEREO_192 = dict(rate_in=192000, rate_out2=48000, mode=2)          # P = 64, the smallest
STEREO_300 = dict(rate_in=300000, rate_out2=48000, mode=2)          # P = 100, the largest
MONO_25 = dict(rate_in=25000, rate_out2=12500, mode=1)              # P = 32, dec_wide
MONO_384 = dict(rate_in=384000, rate_out2=48000, mode=1)            # P = 128
TABLE_CONFIGS = [STEREO_192, STEREO_300, MONO_25, MONO_384]
_answers = {}


def resolved(ask, kw, taps=None):
    """The `t` answer of a configuration (math FAST) as a dict; asked once per configuration."""
    cfg = R.wbfm_config(math=R.MATH_FAST, **kw)
    key = (bytes(cfg), bytes(taps) if taps is not None else None)
    if key not in _answers:
        line, = ask(["t " + " ".join(b.hex() for b in key if b is not None)])
        w = line.split()
        v = list(map(int, w[:97]))
        _answers[key] = dict(cfg=cfg, taps=taps if taps is not None else R.design_taps(cfg), family=v[0], dec_p=v[1], dec_wide=v[2], ci_qf=v[3:6],
                             g_qf=v[6], gq=np.array(v[7:97], dtype=np.int64), table=None if w[97] == "-" else np.frombuffer(bytes.fromhex(w[97]), np.uint8))
    return _answers[key]


def full(half, n):
    """The n taps of a symmetric filter from its n / 2 float taps, exactly, as float64."""
    h = np.array(half[:n // 2], dtype=np.float32).astype(np.float64)
    return np.concatenate([h, h[::-1]])


def quantised(h, qf):
    return np.rint(np.ldexp(h, qf)).astype(np.int64)


def limb_bytes(T, l):
    return (((T + 0x808080) ^ 0x808080) >> (8 * (2 - l))) & 0xFF


def phase_tables(T, P, K0, N):
    """[16][3][N]: byte y of table (r, l) = limb l of T[P - 1 + K0 - r - y], zero outside the filter."""
    out = np.zeros((16, 3, N), dtype=np.uint8)
    y = np.arange(N)
    for r in range(16):
        u = P - 1 + K0 - r - y
        ok = (u >= 0) & (u < len(T))
        for l in range(3):
            out[r, l, ok] = limb_bytes(T[u[ok]], l)
    return out


def exact_composite(fm_half):
    """g = fm * fm (179 taps) from the float taps in exact rational arithmetic."""
    h = [Fraction(float(np.float32(x))) for x in fm_half[:45]]
    h = h + h[::-1]
    return [sum(h[i] * h[u - i] for i in range(max(0, u - 89), min(89, u) + 1)) for u in range(179)]


def is_maximal(taps_times, qf):
    """qf is the largest with max |round(h 2^qf)| <= T_MAX; taps_times(q) = the exact |h| 2^q of the largest tap."""
    return round(taps_times(qf)) <= T_MAX < round(taps_times(qf + 1))


@pytest.mark.parametrize("kw", TABLE_CONFIGS, ids=lambda kw: "%d_%d_mode%d" % (kw["rate_in"], kw["rate_out2"], kw["mode"]))
def test_decimating_tables_equal_the_model(plan_check, kw):
    a = resolved(plan_check, kw)
    stereo = kw["mode"] == 2
    P = 16 * kw["rate_in"] // kw["rate_out2"]
    assert a["family"] == R.MATH_FAST_MFMA_F and a["dec_p"] == P and a["dec_wide"] == int(not stereo and P < 64) and a["table"] is not None
    fm = quantised(full(a["taps"].fm, 90 if stereo else 128), a["ci_qf"][0])
    if stereo:
        g = np.concatenate([a["gq"], a["gq"][:89][::-1]])              # gq[u] = T_g[u] = T_g[178 - u]
        want = np.concatenate([phase_tables(g, P, K0G, DG_N).ravel(), phase_tables(fm, P, K0F, DF_N).ravel()])
    else:
        want = phase_tables(fm, P, K0M, DM_N).ravel()
    assert a["table"].size == want.size and np.array_equal(a["table"], want), np.flatnonzero(a["table"] != want)[:8]


@pytest.mark.parametrize("kw", [STEREO_192, STEREO_300], ids=["192k", "300k"])
def test_composite_taps_are_the_rounded_exact_product(plan_check, kw):
    """|gq[u] - g[u] 2^g_qf| <= 0.5 + 2^-20 with g exact: a bound, since the host sums g in double."""
    a = resolved(plan_check, kw)
    g = exact_composite(a["taps"].fm)
    worst = max(abs(int(a["gq"][u]) - g[u] * 2 ** a["g_qf"]) for u in range(90))
    assert worst <= Fraction(1, 2) + Fraction(1, 2 ** 20), float(worst)


@pytest.mark.parametrize("kw", TABLE_CONFIGS, ids=lambda kw: "%d_%d_mode%d" % (kw["rate_in"], kw["rate_out2"], kw["mode"]))
def test_every_qf_is_the_largest_three_limbs_hold(plan_check, kw):
    a = resolved(plan_check, kw)
    t = a["taps"]
    halves = [(t.fm, 45), (t.fp, 45), (t.fs, 45)] if kw["mode"] == 2 else [(t.fm, 64)]
    for (half, n2), qf in zip(halves, a["ci_qf"]):
        mx = max(Fraction(float(np.float32(x))) for x in map(abs, half[:n2]))
        assert is_maximal(lambda q: mx * 2 ** q, qf), (kw, qf)
        assert np.abs(quantised(full(half, 2 * n2), qf)).max() <= T_MAX
    if kw["mode"] == 2:
        mx = max(map(abs, exact_composite(t.fm)))
        assert is_maximal(lambda q: mx * 2 ** q, a["g_qf"]) and np.abs(a["gq"]).max() <= T_MAX
    else:
        assert a["ci_qf"][1:] == [0, 0] and a["g_qf"] == 0 and not a["gq"].any()


def test_error_estimate_reports_the_qf_of_the_tables(plan_check):
    for kw in TABLE_CONFIGS:
        a = resolved(plan_check, kw)
        e = R.config_error_estimate(a["cfg"])
        assert e["family"] == a["family"]
        if kw["mode"] == 2:
            assert [f["qf"] for f in e["filters"]] == [a["g_qf"], a["ci_qf"][0]] and [f["taps"] for f in e["filters"]] == [179, 90]
        else:
            assert [f["qf"] for f in e["filters"]] == [a["ci_qf"][0]] and [f["taps"] for f in e["filters"]] == [128]
    # a configuration the gate sent down to _MFMA (the composite filter's rms estimate at volume 8) still reports both filters, as the resolver
    # quantised them: fm's qf is in the kernel arguments; g_qf is written only where the composite filter passes, so its qf is the one the same
    # taps have at the default volume
    loud = resolved(plan_check, dict(STEREO_300, volume=8.0))
    e = R.config_error_estimate(loud["cfg"])
    assert loud["family"] == R.MATH_FAST_MFMA == e["family"] and loud["table"] is None and loud["dec_p"] == 0
    assert [f["qf"] for f in e["filters"]] == [resolved(plan_check, STEREO_300)["g_qf"], loud["ci_qf"][0]] and loud["ci_qf"][0] > 0
    assert loud["g_qf"] in (0, e["filters"][0]["qf"])


def test_callers_taps_that_overflow_the_accumulators_resolve_downwards(plan_check):
    """Every limb of fs at its maximum: 128 sum |limb| >= 2^22 - 2^16, so stage C's float-read accumulators cannot hold it - the family is _MFMA, and fs
    (the third filter) is the one left without a qf."""
    cfg = R.wbfm_config(math=R.MATH_FAST, **STEREO_300)
    t = R.design_taps(cfg)
    for k in range(45):
        t.fs[k] = T_MAX / 2 ** 23
    a = resolved(plan_check, STEREO_300, t)
    T = quantised(full(t.fs, 90), 23)
    assert np.abs(T).max() == T_MAX and round(Fraction(T_MAX, 2 ** 23) * 2 ** 24) > T_MAX                       # (23 is its maximal qf)
    assert not 128 * sum(int(np.abs(limb_bytes(T, l).astype(np.int8).astype(np.int64)).sum()) for l in range(3)) < 2 ** 22 - 2 ** 16
    assert a["family"] == R.MATH_FAST_MFMA and a["table"] is None
    assert a["ci_qf"][0] > 0 and a["ci_qf"][1] > 0 and a["ci_qf"][2] == 0
