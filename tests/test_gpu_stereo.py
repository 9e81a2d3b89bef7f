"""Stereo control on the device (fmd_stereo_*; include/fmdemod_mi355x.h, "Stereo control"; csrc/stereo.inc).

Every output byte - the PCM, every field of fmd_stereo_info and of fmd_stereo_meter - is held to tests/stereo_model.py bit for bit, given the
device's own pilot_ms (the RDS tests' manner for phi); pilot_ms itself to the float32 stand-in of the stated summation order bit for bit and to
float64 within (ceil(Mz / 256) + 12) 2^-24 relative.  tests/test_stereo_cpu.py shows that seven planted defects change the model's output on exactly
these inputs (stereo_model.CASES), so the comparisons have teeth.

Shapes, the smallest at which the kernels can go wrong: pcm_stride 8 (one 16-byte word) with lens 0, 1, 2, 7, 8; 1024 and 1032 (128 and 129 words:
threads with and without a word); 2056, one word past a full pass of the 256 threads, so that one thread takes a second word; the stride of a real
batch at block_len 16384; lens above the stride and negative; 1 and 3 streams, 1, 2 and 5 blocks; Mz = 1, 255, 256, 257, 4096 around the 256
threads of the pilot meter."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_model as M   # noqa: E402
import stereo_e2e as E2E   # noqa: E402

pytestmark = pytest.mark.gpu
WORST = {"share": 0.0}        # the largest share of the pilot meter's bound used so far in this session


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def c_config(R, c):
    return R.FmdStereoConfig(c["pcm_stride"], c["pilot_per_block"], c["hold_blocks"], c["reserved0"], c["pilot_on"], c["pilot_off"], c["blend_lo"],
                             c["blend_hi"], c["slew"], (C.c_int32 * 3)(*c["reserved"]))


def make(R, c, S):
    return R.Stereo(c_config(R, c), S)


def to_dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).reshape(-1).copy()).to(torch.device("cuda:0"))


def run_dev(R, st, pcm, lens, z, qual, stream=None, inplace=False, meter=True):
    """one fmd_stereo_run_device call -> (out int16 like pcm, info [S, B], meter [S, B] or None), numpy; stream: a torch stream or None"""
    import torch
    dev = torch.device("cuda:0")
    S, B = lens.shape
    d_pcm = to_dev(pcm, np.int16)
    d_lens = to_dev(lens, np.int32)
    d_z = to_dev(z, np.float32) if z is not None and z.size else None
    d_q = to_dev(qual, np.float32) if qual is not None else None
    d_out = d_pcm if inplace else torch.full_like(d_pcm, 12345)
    d_info = torch.full((S * B * 32,), 0xA5, dtype=torch.uint8, device=dev)
    d_meter = torch.full((S * B * 32,), 0xA5, dtype=torch.uint8, device=dev) if meter else None
    torch.cuda.synchronize()
    st.run_device(d_pcm, d_lens, d_z, d_q, B, d_out, d_info, d_meter, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    st.sync()
    out = d_out.cpu().numpy().reshape(pcm.shape)
    info = d_info.cpu().numpy().view(R.STEREO_INFO_DTYPE).reshape(S, B)
    met = d_meter.cpu().numpy().view(R.STEREO_METER_DTYPE).reshape(S, B) if meter else None
    if not inplace:
        assert np.array_equal(d_pcm.cpu().numpy().reshape(pcm.shape), pcm)          # the input is only read
    return out, info, met


def model(c, states, pcm, lens, info_dev, qual, mode=M.AUTO, with_z=True):
    """the model's launch over the device's own pilot_ms"""
    return M.run(c, states, pcm, lens, info_dev["pilot_ms"].copy() if with_z else None, qual, mode)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_launch(got, want, what):
    for g, w, name in zip(got, want, ("out", "info", "meter")):
        if g is None:
            continue
        if not same(g, w):
            if name == "out":
                bad = np.argwhere(g != w)
                raise AssertionError("%s: out differs at %d values, first [s, b, i] = %s: got %d, want %d" % (what, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))
            for f in g.dtype.names:
                assert same(np.ascontiguousarray(g[f]), np.ascontiguousarray(w[f])), (what, name, f, g[f], w[f])
            raise AssertionError((what, name))


def pilot_standin(c, z):
    inv = M.plan(c)["inv_mz"]
    return np.array([[M.pilot_ms(z[s, b], inv) for b in range(z.shape[1])] for s in range(z.shape[0])], dtype=np.float32)


# ---- 1. against the model, bit for bit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(M.CASES) + ["sweep@batch"])
def test_out_info_and_meters_equal_the_model(R, name):
    stride = None
    if name.endswith("@batch"):
        b = R.BatchDemod(R.wbfm_config(rate_in=300000, rate_out2=48000, mode=2, block_len=16384, math=R.MATH_FAST), 1)
        stride = b.pcm_stride
        b.close()
        assert stride % 8 == 0 and stride not in (8, 1024, 1032)
    c, pcm, lens, z, qual = M.case_inputs(name.split("@")[0], stride)
    S, B = lens.shape
    st = make(R, c, S)
    got = run_dev(R, st, pcm, lens, z, qual)
    states = [M.new_state() for _ in range(S)]
    want = model(c, states, pcm, lens, got[1], qual)
    assert same(got[1]["pilot_ms"], pilot_standin(c, z)), (got[1]["pilot_ms"], pilot_standin(c, z))
    assert_launch(got, want, name)
    for s in range(S):
        d = st.get_state(s)
        assert (np.float32(d.g).tobytes(), d.stereo, d.run, d.reserved) == (np.float32(states[s]["g"]).tobytes(), states[s]["stereo"], states[s]["run"], 0), s
    # beyond the frames every value is the input's; a closed block is untouched
    for s in range(S):
        for b in range(B):
            n = int(got[1]["frames"][s, b])
            assert n == min(max(int(lens[s, b]), 0), c["pcm_stride"]) // 2
            assert np.array_equal(got[0][s, b, 2 * n:], pcm[s, b, 2 * n:])
    if name == "sweep":
        assert np.array_equal(got[0][0, 4], pcm[0, 4]) and got[1]["g_start"][0, 4] == 1 and got[1]["g_end"][0, 4] == 1      # g = 1: the identity
        n = int(got[1]["frames"][0, 2])
        assert got[1]["g_end"][0, 2] == 0 and np.array_equal(got[0][0, 2, 2 * n - 2], got[0][0, 2, 2 * n - 1])               # the ramp ends in mono
    st.close()


@pytest.mark.parametrize("mz", E2E.PILOT_SIZES)
def test_pilot_ms_equals_the_stated_order_and_meets_its_bound(R, mz):
    S, B = 2, 2
    c = M.config(pcm_stride=8, pilot_per_block=mz, hold_blocks=1)
    z = np.concatenate([M.pilot_z(1, 1, mz, [[0.3]], seed=mz), M.pilot_z(1, 3, mz, [[0.01, 0.15, 1.7]], seed=mz + 1).reshape(3, 1, mz, 2)]).reshape(S, B, mz, 2)
    pcm = M.lcg_pcm(S, B, 8)
    lens = np.full((S, B), 8, dtype=np.int32)
    st = make(R, c, S)
    _, info, _ = run_dev(R, st, pcm, lens, z, None)
    st.close()
    assert same(info["pilot_ms"], pilot_standin(c, z)), (info["pilot_ms"], pilot_standin(c, z))
    for s in range(S):
        for b in range(B):
            exact = M.pilot_ms_f64(z[s, b])
            share = abs(float(info["pilot_ms"][s, b]) - exact) / M.pilot_bound(mz, exact)
            WORST["share"] = max(WORST["share"], share)
            print("Mz %d [%d, %d]: pilot_ms %.9g, exact %.9g, share of the bound %.4f (largest so far %.4f)" % (mz, s, b, info["pilot_ms"][s, b], exact, share, WORST["share"]))
            assert share <= 1, (mz, s, b, share)
    assert M.pilot_bound(mz, 1.0) == (math.ceil(mz / 256) + 12) * 2.0 ** -24 + 2.0 ** -126


# ---- 2. independence ------------------------------------------------------------------------------------------------------------------------

def whole_of(R, name):
    c, pcm, lens, z, qual = M.case_inputs(name)
    st = make(R, c, lens.shape[0])
    got = run_dev(R, st, pcm, lens, z, qual)
    return c, pcm, lens, z, qual, st, got


def cat(parts):
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(3))


@pytest.mark.parametrize("name", ["hold", "sweep"])
def test_split_in_place_and_stream_count_change_nothing(R, name):
    c, pcm, lens, z, qual, st, whole = whole_of(R, name)
    S = lens.shape[0]
    st.reset()
    parts = cat([run_dev(R, st, pcm[:, :2], lens[:, :2], z[:, :2], qual[:, :2]), run_dev(R, st, pcm[:, 2:], lens[:, 2:], z[:, 2:], qual[:, 2:])])
    assert_launch(parts, whole, "5 blocks = 2 + 3")
    st.reset()
    assert_launch(run_dev(R, st, pcm, lens, z, qual, inplace=True), whole, "in place")
    st.reset()
    assert_launch(run_dev(R, st, pcm, lens, z, qual, meter=False), whole, "without meters")
    st.close()
    one = make(R, c, 1)
    for s in range(S):
        one.reset()
        assert_launch(run_dev(R, one, pcm[s:s + 1], lens[s:s + 1], z[s:s + 1], qual[s:s + 1]), tuple(w[s:s + 1] for w in whole), "stream %d alone" % s)
    one.close()


def test_a_launch_on_a_second_stream_is_handed_over(R):
    import torch
    c, pcm, lens, z, qual, st, whole = whole_of(R, "hold")
    st.reset()
    ts = torch.cuda.Stream()
    a = run_dev(R, st, pcm[:, :2], lens[:, :2], z[:, :2], qual[:, :2], stream=ts)
    b = run_dev(R, st, pcm[:, 2:4], lens[:, 2:4], z[:, 2:4], qual[:, 2:4])
    d = run_dev(R, st, pcm[:, 4:], lens[:, 4:], z[:, 4:], qual[:, 4:], stream=ts)
    assert_launch(cat([a, b, d]), whole, "caller's stream, own stream, caller's stream")
    st.close()


def test_state_round_trip_and_reset(R):
    c, pcm, lens, z, qual, st, whole = whole_of(R, "hold")
    S = lens.shape[0]
    st.reset()
    first = run_dev(R, st, pcm[:, :3], lens[:, :3], z[:, :3], qual[:, :3])
    states = [st.get_state(s) for s in range(S)]
    assert any(s.g != 0 for s in states) and all(s.stereo == 1 for s in states[:1])
    fresh = make(R, c, S)
    for s in range(S):
        fresh.set_state(s, states[s])
    rest = run_dev(R, fresh, pcm[:, 3:], lens[:, 3:], z[:, 3:], qual[:, 3:])
    assert_launch(cat([first, rest]), whole, "continued from get_state / set_state")
    L = R.lib()
    for bad in (R.FmdStereoState(1.5, 0, 0, 0), R.FmdStereoState(float("nan"), 0, 0, 0), R.FmdStereoState(0.5, 2, 0, 0), R.FmdStereoState(0.5, 1, c["hold_blocks"], 0),
                R.FmdStereoState(0.5, 1, -1, 0), R.FmdStereoState(0.5, 1, 0, 1)):
        assert L.fmd_stereo_set_state(fresh._h, 0, C.byref(bad)) == M.E_ARG
    assert L.fmd_stereo_get_state(fresh._h, S, C.byref(bad)) == M.E_ARG
    fresh.reset()
    for s in range(S):
        assert not any(bytes(fresh.get_state(s)))            # mono, g = 0
    assert_launch(run_dev(R, fresh, pcm, lens, z, qual), whole, "after reset")
    fresh.close()
    st.close()


# ---- 3. graph -------------------------------------------------------------------------------------------------------------------------------

def test_a_captured_graph_replays_to_the_bits_of_plain_launches(R):
    """One torch stream, no branches: the three kernels of a one-block launch captured once and replayed three times with the inputs refilled.  The
    state advances in place, so replay r continues replay r - 1; the mode is the captured one whatever set_mode says later.  A launch whose stream
    differs from the previous launch's is refused inside a capture (FMD_E_STATE) and leaves the capture valid."""
    import torch
    c, pcm, lens, z, qual, eager, whole = whole_of(R, "hold")
    eager.close()
    S, reps = lens.shape[0], 3
    dev = torch.device("cuda:0")
    g_obj = make(R, c, S)
    d_pcm = torch.zeros(S * c["pcm_stride"], dtype=torch.int16, device=dev)
    d_out = torch.zeros_like(d_pcm)
    d_lens = torch.zeros(S, dtype=torch.int32, device=dev)
    d_z = torch.zeros(S * c["pilot_per_block"] * 2, dtype=torch.float32, device=dev)
    d_q = torch.zeros(S, dtype=torch.float32, device=dev)
    d_info = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
    d_meter = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=ts):
        g_obj.run_device(d_pcm, d_lens, d_z, d_q, 1, d_out, d_info, d_meter, hip_stream=ts.cuda_stream)
    g_obj.set_mode(R.STEREO_FORCE_MONO)                     # the captured launch keeps FMD_STEREO_AUTO
    for r in range(reps):
        d_pcm.copy_(to_dev(pcm[:, r], np.int16))
        d_lens.copy_(to_dev(lens[:, r], np.int32))
        d_z.copy_(to_dev(z[:, r], np.float32))
        d_q.copy_(to_dev(qual[:, r], np.float32))
        d_out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (d_out.cpu().numpy().reshape(S, 1, -1), d_info.cpu().numpy().view(R.STEREO_INFO_DTYPE).reshape(S, 1),
               d_meter.cpu().numpy().view(R.STEREO_METER_DTYPE).reshape(S, 1))
        assert_launch(got, tuple(w[:, r:r + 1] for w in whole), "replay %d" % r)
    g_obj.set_mode(R.STEREO_AUTO)
    # the previous launch on another stream: no event hand-over inside a capture
    g_obj.run_device(d_pcm, d_lens, d_z, d_q, 1, d_out, d_info, d_meter)              # the object's own stream
    g2 = torch.cuda.CUDAGraph()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.graph(g2, stream=ts):
        rc = R.lib().fmd_stereo_run_device(g_obj._h, p(d_pcm), p(d_lens), p(d_z), p(d_q), 1, p(d_out), p(d_info), p(d_meter), C.c_void_p(ts.cuda_stream))
        msg = R.lib().fmd_last_error().decode()
        d_q.fill_(3.0)
    assert rc == M.E_STATE and "fmd_stereo_sync" in msg, (rc, msg)
    g_obj.sync()
    g2.replay()
    torch.cuda.synchronize()
    assert bool((d_q == 3.0).all())
    g_obj.close()


# ---- 4. modes, arguments, the host form --------------------------------------------------------------------------------------------------------

def test_forced_modes_need_no_pilot_and_auto_refuses_without_one(R):
    import torch
    c, pcm, lens, z, qual = M.case_inputs("hold")
    S, B = lens.shape
    st = make(R, c, S)
    L = R.lib()
    for mode in (R.STEREO_FORCE_STEREO, R.STEREO_FORCE_MONO, R.STEREO_FORCE_STEREO):         # g: up by slew a block, down again, up again
        st.set_mode(mode)
        states = [st.get_state(s) for s in range(S)]
        got = run_dev(R, st, pcm, lens, None, None)
        ms = [dict(g=np.float32(x.g), stereo=x.stereo, run=x.run) for x in states]
        assert_launch(got, M.run(c, ms, pcm, lens, None, None, mode), "mode %d" % mode)
        assert not got[1]["pilot_ms"].any() and not got[1]["stereo"].any()
    # with a pilot given, a forced mode still reports it and leaves the indicator alone
    st.set_mode(R.STEREO_FORCE_MONO)
    got = run_dev(R, st, pcm, lens, z, qual)
    assert same(got[1]["pilot_ms"], pilot_standin(c, z)) and not got[1]["stereo"].any()
    mono = got[0][:, -1]
    n = int(got[1]["frames"][0, -1])
    assert got[1]["g_end"][0, -1] == 0 and np.array_equal(mono[0, 2 * n - 2], mono[0, 2 * n - 1])
    st.set_mode(R.STEREO_AUTO)
    d = to_dev(np.zeros(S * B * c["pcm_stride"] + 64), np.int16)
    d_i = torch.zeros(S * B * 32 + 64, dtype=torch.uint8, device=d.device)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), None, None, B, p(d), p(d_i), None, None) == M.E_ARG and b"AUTO" in L.fmd_last_error()
    assert L.fmd_stereo_set_mode(st._h, 3) == M.E_ARG and L.fmd_stereo_set_mode(st._h, -1) == M.E_ARG
    st.set_mode(R.STEREO_FORCE_MONO)
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), None, None, B, p(d, 16), p(d_i), None, None) == M.E_ARG and b"overlaps" in L.fmd_last_error()
    assert L.fmd_stereo_run_device(st._h, p(d, 8), p(d_i), None, None, B, p(d, 8), p(d_i), None, None) == M.E_ARG and b"16-byte" in L.fmd_last_error()
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), None, None, B, p(d), None, None, None) == M.E_ARG
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), None, None, -1, p(d), p(d_i), None, None) == M.E_ARG
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), None, None, 0, p(d), p(d_i), None, None) == 0
    st.close()
    # pilot_per_block 0: forced modes only
    c0 = M.config(pcm_stride=c["pcm_stride"], pilot_per_block=0, hold_blocks=c["hold_blocks"], slew=c["slew"])
    st = make(R, c0, S)
    assert L.fmd_stereo_run_device(st._h, p(d), p(d_i), p(d), None, B, p(d), p(d_i), None, None) == M.E_ARG
    st.set_mode(R.STEREO_FORCE_STEREO)
    got = run_dev(R, st, pcm, lens, None, qual)
    assert_launch(got, M.run(c0, [M.new_state() for _ in range(S)], pcm, lens, None, qual, M.FORCE_STEREO), "Mz = 0")
    st.close()


@pytest.mark.parametrize("name", ["hold", "tiny"])
def test_the_host_form_equals_the_device_form(R, name):
    c, pcm, lens, z, qual, st, whole = whole_of(R, name)
    st.reset()
    zc = z.view(np.complex64)[..., 0]
    a = st.run_host(pcm[:, :3], lens[:, :3], zc[:, :3], qual[:, :3], 3)
    b = st.run_host(pcm[:, 3:], lens[:, 3:], zc[:, 3:], qual[:, 3:], 2)                      # (the staging shrinks: kept)
    assert_launch(cat([a, b]), whole, "host form, 3 + 2 blocks")
    st.reset()
    mixed = cat([st.run_host(pcm[:, :2], lens[:, :2], zc[:, :2], qual[:, :2], 2), run_dev(R, st, pcm[:, 2:], lens[:, 2:], z[:, 2:], qual[:, 2:])])
    assert_launch(mixed, whole, "host then device form")
    st.close()


# ---- 5. end to end with the demodulator and the 19 kHz receiver ----------------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [1, 0])
def test_end_to_end_on_the_dds_multiplex(R, stereo):
    """u8 IQ of the oracle's DDS multiplex through a FMD_MATH_FAST stereo batch with the v tap and levels, Batch.subcarrier(19000, 500) on the tap,
    Batch.stereo on its z and the levels.  Thresholds from the float64 chain (tests/stereo_e2e.py; tests/test_stereo_cpu.py asserts the factor of
    100 between the two inputs).  With the pilot the indicator turns on at block hold_blocks - 1 and stays on, and once g = 1 the output is the
    batch's PCM; without it the indicator never turns on and L == R in every frame."""
    import torch
    bl, nb, hold = E2E.BLOCK_LEN, E2E.N_BLOCKS, E2E.HOLD
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(E2E.dds_iq(stereo).copy()).to(dev)
    b = R.BatchDemod(R.wbfm_config(rate_in=E2E.RATE, rate_out2=48000, mode=2, block_len=bl, math=R.MATH_FAST), 1)
    pcm = torch.zeros(nb * b.pcm_stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(nb, dtype=torch.int32, device=dev)
    levels = torch.zeros(nb, dtype=torch.float32, device=dev)
    v = torch.zeros((1, nb, bl // 16), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.run_device_levels(iq, nb, pcm, lens, levels, debug={"v": v})
    b.sync()
    sub = b.subcarrier(E2E.FC, E2E.BW, n_taps=E2E.N_TAPS, decim=E2E.DECIM)
    z = torch.zeros((1, nb, sub.out_per_block, 2), dtype=torch.float32, device=dev)
    sub.run_device(v, nb, z)
    sub.sync()
    p_on, p_off = E2E.thresholds()
    st = b.stereo(sub, R.FmdStereoConfig(0, 0, hold, 0, p_on, p_off, 0.05, 0.25, 1.0))
    assert (st.cfg.pcm_stride, st.cfg.pilot_per_block, st.n_streams) == (b.pcm_stride, sub.out_per_block, 1)
    out = torch.zeros_like(pcm)
    info = torch.zeros(nb * 32, dtype=torch.uint8, device=dev)
    meter = torch.zeros(nb * 32, dtype=torch.uint8, device=dev)
    st.run_device(pcm, lens, z, levels, nb, out, info, meter)
    st.sync()
    pcm_np, out_np = pcm.cpu().numpy().reshape(1, nb, -1), out.cpu().numpy().reshape(1, nb, -1)
    lens_np, lev_np = lens.cpu().numpy().reshape(1, nb), levels.cpu().numpy().reshape(1, nb)
    info_np = info.cpu().numpy().view(R.STEREO_INFO_DTYPE).reshape(1, nb)
    meter_np = meter.cpu().numpy().view(R.STEREO_METER_DTYPE).reshape(1, nb)
    print("stereo=%d: pilot_ms %s (float64 chain %s), thresholds^2 on %.3g off %.3g, levels %s, g_end %s" %
          (stereo, info_np["pilot_ms"][0], E2E.pilot_ms_f64_of_dds(stereo), p_on ** 2, p_off ** 2, lev_np[0], info_np["g_end"][0]))
    c = M.config(b.pcm_stride, sub.out_per_block, hold, p_on, p_off, 0.05, 0.25, 1.0)
    assert_launch((out_np, info_np, meter_np), model(c, [M.new_state()], pcm_np, lens_np, info_np, lev_np), "end to end")
    assert lens_np.min() > 0 and (lev_np > 0.25).all()
    if stereo:
        assert list(info_np["stereo"][0]) == [0] * (hold - 1) + [1] * (nb - hold + 1)
        assert list(info_np["g_end"][0]) == [0.0] * (hold - 1) + [1.0] * (nb - hold + 1)
        assert np.array_equal(out_np[0, hold:], pcm_np[0, hold:]) and not np.array_equal(out_np[0, 0], pcm_np[0, 0])
        assert (pcm_np[0, hold:, 0::2] != pcm_np[0, hold:, 1::2]).any()                    # there is a stereo image to keep
    else:
        assert not info_np["stereo"].any() and not info_np["g_end"].any()
        for k in range(nb):
            n = int(info_np["frames"][0, k])
            assert n == lens_np[0, k] // 2 and np.array_equal(out_np[0, k, 0:2 * n:2], out_np[0, k, 1:2 * n:2])
    st.close()
    sub.close()
    b.close()
