"""Channel level and power squelch on the device (fmd_batch_run_device_levels / _run_host_levels / _set_squelch; include/fmdemod_mi355x.h,
"Channel level and power squelch").

The level of a block is the reference's rms() over its lowpassed buffer (float64 model: tests/levels_model.py).  It is checked against the
oracle's decimated signal and against the same launch's `y` debug tap; it must not depend on how a launch is cut into time chunks, on how the
blocks are split into launches or on the stream's neighbours; a levels launch must leave PCM, lengths and state exactly as a plain launch does;
and squelch must close exactly the blocks the recurrence over the returned levels closes, leaving everything else bit-identical."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from levels_model import block_level, squelch_model  # noqa: E402
from test_gpu_parity import CONFIGS  # noqa: E402

pytestmark = pytest.mark.gpu

BL = 262144
NB = 8
MATHS = ["exact", "valu", "mfma", "mfma_f"]


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def math_of(R, name):
    return {"exact": R.MATH_EXACT, "valu": R.MATH_FAST_VALU, "mfma": R.MATH_FAST_MFMA, "mfma_f": R.MATH_FAST_MFMA_F}[name]


@functools.lru_cache(maxsize=None)
def iq_of(kind, n_bytes):
    from oracle import dds_bytes, lcg_bytes
    if kind == "lcg":
        return lcg_bytes(n_bytes, 12345)[0]
    if kind == "dds":
        return dds_bytes(n_bytes, amp=100)
    if kind == "quiet":                                   # no antenna: one LSB of ADC noise (the exact-tile path of the fast kernels)
        return np.random.default_rng(7).integers(127, 129, n_bytes, dtype=np.uint8)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def oracle_levels(kw_items, kind, block_len, nb):
    """[(level, S2 / n)] per block from the oracle's trace of the decimated signal."""
    from oracle import OracleStream
    kw = dict(kw_items)
    s = OracleStream(**kw)
    iq = iq_of(kind, nb * block_len)
    return [block_level(s.block(iq[k * block_len:(k + 1) * block_len], trace=True)[1]["y"]) for k in range(nb)]


def assert_levels_close(got, want):
    """|lvl_gpu^2 - lvl_ref^2| <= 1e-5 S2/n + 1e-12, block by block."""
    for k, (g, (lvl, ms)) in enumerate(zip(got, want)):
        g = float(g)
        assert abs(g * g - lvl * lvl) <= 1e-5 * ms + 1e-12, "block %d: gpu level %.9g, oracle %.9g (S2/n %.6g)" % (k, g, lvl, ms)


def levels_host(R, kw, kind, math, block_len=BL, nb=NB, n_streams=1):
    b = R.BatchDemod(R.wbfm_config(block_len=block_len, math=math, **kw), n_streams)
    iq = np.tile(iq_of(kind, nb * block_len), n_streams).reshape(n_streams, nb, block_len)
    pcm, lens, lv = b.run_host_levels(iq, nb)
    b.close()
    return pcm, lens, lv


@pytest.mark.parametrize("kind", ["lcg", "dds"])
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_level_matches_the_oracle(R, name, math, kind):
    _, _, lv = levels_host(R, CONFIGS[name], kind, math_of(R, math))
    assert_levels_close(lv[0], oracle_levels(tuple(sorted(CONFIGS[name].items())), kind, BL, NB))


EXTRA = {
    "offset_tuning": (dict(rate_in=300000, rate_out2=48000, mode=2, offset_tuning=True), BL),
    "mode0_drop": (dict(rate_in=300000, rate_out2=48000, mode=0), BL),
    "ragged_200000": (dict(rate_in=300000, rate_out2=48000, mode=2), 200000),
    "ragged_mono_200000": (dict(rate_in=300000, rate_out2=48000, mode=1), 200000),
}


@pytest.mark.parametrize("kind", ["lcg", "dds"])
@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("name", sorted(EXTRA))
def test_level_matches_the_oracle_offset_tuning_mode0_ragged(R, name, math, kind):
    kw, block_len = EXTRA[name]
    m = R.MATH_EXACT if math == "exact" else R.MATH_FAST
    _, _, lv = levels_host(R, kw, kind, m, block_len=block_len)
    assert_levels_close(lv[0], oracle_levels(tuple(sorted(kw.items())), kind, block_len, NB))


def device_run(R, b, iq_np, nb, levels=True, taps=False):
    """one device launch of b over iq_np [S, nb, BL]: (pcm, lens, levels or None, y tap or None) as numpy"""
    import torch
    dev = torch.device("cuda:0")
    S = b.n_streams
    M = b.cfg.block_len // 16
    iq = torch.from_numpy(np.ascontiguousarray(iq_np).reshape(-1)).to(dev)
    pcm = torch.zeros(S * nb * b.pcm_stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(S * nb, dtype=torch.int32, device=dev)
    lv = torch.full((S, nb), -1.0, dtype=torch.float32, device=dev) if levels else None
    y = torch.zeros(S * nb * 2 * M, dtype=torch.float32, device=dev) if taps else None
    torch.cuda.synchronize()
    if levels:
        b.run_device_levels(iq, nb, pcm, lens, lv, debug={"y": y} if taps else None)
    else:
        b.run_device(iq, nb, pcm, lens, debug={"y": y} if taps else None)
    b.sync()
    out = (pcm.cpu().numpy().reshape(S, nb, -1), lens.cpu().numpy().reshape(S, nb),
           lv.cpu().numpy() if levels else None, y.cpu().numpy().reshape(S, nb, 2 * M) if taps else None)
    return out


@pytest.mark.parametrize("kind", ["lcg", "quiet"])
@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "mono_300k"])
def test_level_matches_the_launch_own_y_and_the_plain_build(R, name, math, kind):
    """One run_device_levels launch with a y tap (the DBG, LV build): its levels match the tap's y at the oracle tolerance; the build without
    taps (DBG = false, LV) gives bit-identical levels."""
    nb = 4
    iq = iq_of(kind, nb * BL).reshape(1, nb, BL)
    cfg = R.wbfm_config(math=math_of(R, math), **CONFIGS[name])
    b = R.BatchDemod(cfg, 1)
    _, _, lv_dbg, y = device_run(R, b, iq, nb, taps=True)
    b.close()
    assert_levels_close(lv_dbg[0], [block_level(y[0, k]) for k in range(nb)])
    b = R.BatchDemod(cfg, 1)
    _, _, lv, _ = device_run(R, b, iq, nb)
    b.close()
    assert np.array_equal(lv.view(np.uint32), lv_dbg.view(np.uint32)), (lv, lv_dbg)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "mono_300k", "nfm_25k"])
def test_levels_do_not_depend_on_time_split_or_launch_split(R, name, math):
    iq = iq_of("lcg", NB * BL).reshape(1, NB, BL)
    cfg = R.wbfm_config(math=math_of(R, math), **CONFIGS[name])
    got = {}
    for split in (-1, 0, 48):
        b = R.BatchDemod(cfg, 1)
        b.set_time_split(split)
        got[split] = b.run_host_levels(iq, NB)[2]
        b.close()
    b = R.BatchDemod(cfg, 1)
    halves = [b.run_host_levels(np.ascontiguousarray(iq[:, h * 4:(h + 1) * 4]), 4)[2] for h in range(2)]
    b.close()
    got["4+4"] = np.concatenate(halves, axis=1)
    ref = got[0].view(np.uint32)
    bad = {k: v for k, v in got.items() if not np.array_equal(v.view(np.uint32), ref)}
    assert not bad, "levels differ from the default split's %s: %s" % (got[0], bad)


@pytest.mark.parametrize("math", MATHS)
def test_levels_of_a_stream_alone_and_as_stream_37_of_256(R, math):
    import torch
    nb = 2
    cfg = R.wbfm_config(math=math_of(R, math), **CONFIGS["stereo_300k"])
    iq1 = iq_of("dds", nb * BL).reshape(1, nb, BL)
    b = R.BatchDemod(cfg, 1)
    alone = device_run(R, b, iq1, nb)[2]
    b.close()
    g = torch.Generator().manual_seed(5)
    many = torch.randint(0, 256, (256, nb, BL), dtype=torch.uint8, generator=g).numpy()
    many[37] = iq1[0]
    b = R.BatchDemod(cfg, 256)
    lv = device_run(R, b, many, nb)[2]
    b.close()
    assert np.array_equal(lv[37].view(np.uint32), alone[0].view(np.uint32)), (lv[37], alone[0])


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", ["stereo_300k", "mono_300k", "nfm_25k"])
def test_a_levels_launch_does_not_perturb(R, name, math):
    """squelch off: PCM, lengths and the carried state of a levels launch are bit-identical to a plain launch of the same family"""
    nb = 4
    iq = iq_of("lcg", nb * BL).reshape(1, nb, BL)
    cfg = R.wbfm_config(math=math_of(R, math), **CONFIGS[name])
    res = []
    for levels in (False, True):
        b = R.BatchDemod(cfg, 1)
        pcm, lens, _, _ = device_run(R, b, iq, nb, levels=levels)
        res.append((pcm, lens, bytes(b.get_state(0))))
        b.close()
    (p0, l0, s0), (p1, l1, s1) = res
    assert np.array_equal(l0, l1)
    for k in range(nb):
        assert np.array_equal(p0[0, k, :l0[0, k]], p1[0, k, :l1[0, k]]), k
    assert s0 == s1


# ---- squelch --------------------------------------------------------------------------------------------------------------------------

PATTERN = "LQQQLQLQ"      # per block, rolled by the stream index: loud (dds amp 100) or quiet (127 / 128)


def squelch_input():
    loud, quiet = iq_of("dds", NB * BL).reshape(NB, BL), iq_of("quiet", NB * BL).reshape(NB, BL)
    iq = np.empty((4, NB, BL), np.uint8)
    for s in range(4):
        pat = PATTERN[s:] + PATTERN[:s]
        for k in range(NB):
            iq[s, k] = loud[k] if pat[k] == "L" else quiet[k]
    return iq


def run_pump(R, b, iq, per):
    L = R.lib()
    S = b.n_streams
    rings = []
    for s in range(S):
        h = C.c_void_p()
        assert L.fmd_ingest_create(C.byref(h), b._h, s, 0) == 0
        rings.append(h)
    pcm_all, lens_all = [], []
    try:
        for c in range(NB // per):
            for s in range(S):
                chunk = np.ascontiguousarray(iq[s, c * per:(c + 1) * per]).reshape(-1)
                L.fmd_ingest_callback(chunk.ctypes.data, chunk.size, rings[s])
            pcm = np.zeros((S, per, b.pcm_stride), np.int16)
            lens = np.zeros((S, per), np.int32)
            assert L.fmd_batch_pump(b._h, per, pcm.ctypes.data, lens.ctypes.data) == per
            pcm_all.append(pcm)
            lens_all.append(lens)
    finally:
        b.sync()
        for h in rings:
            L.fmd_ingest_destroy(h)
    return np.concatenate(pcm_all, axis=1), np.concatenate(lens_all, axis=1)


def run_split(R, b, iq, per, path):
    """(pcm, lens, levels or None) of NB blocks in launches of `per` blocks through one of the run paths"""
    if path == "pump":
        return run_pump(R, b, iq, per) + (None,)
    parts = []
    for c in range(NB // per):
        x = np.ascontiguousarray(iq[:, c * per:(c + 1) * per])
        parts.append(b.run_host_levels(x, per) if path == "host_levels" else b.run_host(x, per) + (None,))
    lv = None if path == "host" else np.concatenate([p[2] for p in parts], axis=1)
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1), lv


@pytest.mark.parametrize("path", ["host", "host_levels", "pump"])
@pytest.mark.parametrize("per", [8, 4])
@pytest.mark.parametrize("conseq", [0, 2])
@pytest.mark.parametrize("math", ["exact", "fast"])
def test_squelch(R, math, conseq, per, path):
    cfg = R.wbfm_config(math=R.MATH_EXACT if math == "exact" else R.MATH_FAST, **CONFIGS["stereo_300k"])
    iq = squelch_input()
    # the unsquelched run with the same launch split: levels, PCM, lengths, state
    b = R.BatchDemod(cfg, 4)
    p0, l0, lv0 = run_split(R, b, iq, per, "host_levels")
    st0 = [bytes(b.get_state(s)) for s in range(4)]
    b.close()
    pats = [PATTERN[s:] + PATTERN[:s] for s in range(4)]
    loud = [lv0[s, k] for s in range(4) for k in range(NB) if pats[s][k] == "L"]
    quiet = [lv0[s, k] for s in range(4) for k in range(NB) if pats[s][k] == "Q"]
    t = float(np.sqrt(max(quiet) * min(loud)))
    assert max(quiet) < t < min(loud), (quiet, loud)
    thr = np.array([0.0, t, 1e3, t], np.float32)
    want_closed, want_hits = squelch_model(lv0, thr, conseq)
    assert want_closed[1].any() and not want_closed[1].all() and want_closed[2].all() and not want_closed[0].any()

    b = R.BatchDemod(cfg, 4)
    b.set_squelch(thr, conseq)
    assert [b.squelch_hits(s) for s in range(4)] == [conseq + 1] * 4
    pcm, lens, lv = run_split(R, b, iq, per, path)
    if lv is not None:
        assert np.array_equal(lv.view(np.uint32), lv0.view(np.uint32))
    for s in range(4):
        for k in range(NB):
            if want_closed[s, k]:
                assert lens[s, k] == 0 and not pcm[s, k].any(), (s, k)
            else:
                assert lens[s, k] == l0[s, k] and np.array_equal(pcm[s, k, :lens[s, k]], p0[s, k, :l0[s, k]]), (s, k)
        assert bytes(b.get_state(s)) == st0[s], s
    assert [b.squelch_hits(s) for s in range(4)] == [conseq + 1 if thr[s] <= 0 else want_hits[s] for s in range(4)]
    b.set_squelch_hits(1, 0)
    assert b.squelch_hits(1) == 0
    b.reset()
    assert [b.squelch_hits(s) for s in range(4)] == [conseq + 1] * 4
    b.close()


def test_squelch_argument_checks(R):
    from rtl_fm_player_amd import FmdError
    b = R.BatchDemod(R.wbfm_config(**CONFIGS["stereo_300k"]), 2)
    with pytest.raises(FmdError):
        b.squelch_hits(0)                                                    # never set: FMD_E_STATE
    with pytest.raises(FmdError):
        b.set_squelch([1.0, 1.0], conseq=-1)
    with pytest.raises(FmdError):
        b.set_squelch([1.0, float("nan")])
    with pytest.raises(FmdError):
        b.set_squelch([1.0, float("inf")])
    b.set_squelch([1.0, 0.0], conseq=3)
    for bad in ((2, 0), (-1, 0), (0, -1), (0, 5)):
        with pytest.raises(FmdError):
            b.set_squelch_hits(*bad)
    with pytest.raises(FmdError):
        b.squelch_hits(2)
    assert b.squelch_hits(0) == 4 and b.squelch_hits(1) == 4
    b.set_squelch(None)
    b.close()


def test_levels_and_squelch_inside_a_captured_graph(R):
    """The finish kernel is a plain launch on the captured stream: a replayed graph gives the levels and the squelch of a direct launch."""
    import torch
    nb = 2
    cfg = R.wbfm_config(math=R.MATH_FAST, **CONFIGS["stereo_300k"])
    iq_np = squelch_input()[:, :nb]
    dev = torch.device("cuda:0")
    want = []
    for graph in (False, True):
        b = R.BatchDemod(cfg, 4)
        b.set_timing(False)
        b.set_squelch(np.array([0.0, 1e-3, 1e3, 1e-3], np.float32), 0)
        iq = torch.from_numpy(np.ascontiguousarray(iq_np).reshape(-1)).to(dev)
        pcm = torch.zeros(4 * nb * b.pcm_stride, dtype=torch.int16, device=dev)
        lens = torch.zeros(4 * nb, dtype=torch.int32, device=dev)
        lv = torch.zeros((4, nb), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if graph:
            b.run_device_levels(iq, nb, pcm, lens, lv)                        # sizes the level scratch outside the capture
            b.sync()
            b.reset()
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                b.run_device_levels(iq, nb, pcm, lens, lv, hip_stream=s.cuda_stream)
            g.replay()
            torch.cuda.synchronize()
        else:
            b.run_device_levels(iq, nb, pcm, lens, lv)
            b.sync()
        want.append((pcm.cpu().numpy(), lens.cpu().numpy(), lv.cpu().numpy(), [b.squelch_hits(k) for k in range(4)]))
        b.close()
    (p0, l0, v0, h0), (p1, l1, v1, h1) = want
    assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(l0, l1) and np.array_equal(p0, p1) and h0 == h1
