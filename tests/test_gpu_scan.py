"""The station finder (fmd_scan_*, csrc/scan.inc) on the device against tests/scan_model.py, the definition in float64.

Synthetic spectra are handed in directly - the fixed cases of scan_model.CASES, whose decision margins tests/test_scan_cpu.py asserts from the model
alone - and held to scan_model.assert_matches: found, written, candidate and offset_hz equal; power, snr and d_chan within one float32 ulp of the
model's rounded value; centroid_hz within 2^-23 max(|centroid_hz|, bw); the slots beyond `written` all-zero bytes.  Then bit equality of every output
wherever the header says the result depends on the launch's d_power and the configuration alone: a stream alone and among others, a caller's stream,
a captured graph replayed twice, the host form.  Last the chain spectrum -> scan -> fmd_tuner_shift -> tuner -> spectrum -> scan on a capture, whose
expectation tests/test_scan_cpu.py shows with the models first.

Shapes: n_bins 64, 256 and 4096; 1 and 3 blocks; 1 and 5 streams; 21 to 959 candidates (one to four per thread)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

FMD_E_ARG = -1


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def c_config(R, cfg):
    return R.FmdScanConfig(cfg["rate"], cfg["n_bins"], cfg["raster_hz"], cfg["bw"], cfg["min_sep"], cfg["floor_permille"], cfg["dc_guard"],
                           cfg["max_stations"], cfg["threshold"], (C.c_int32 * 3)(*cfg["reserved"]))


_MODEL = {}


def case(name):
    """(configuration, power, the model's results) of a fixed case: made once, shared, read-only"""
    if name not in _MODEL:
        _, cfg, n_blocks, n_streams, kind, _ = next(c for c in M.CASES if c[0] == name)
        power = M.case_power(kind, cfg, n_blocks, n_streams)
        _MODEL[name] = (cfg, power, M.scan(power, cfg))
    return _MODEL[name]


def run_dev(scan, power, want_chan=True, stream=None):
    """one fmd_scan_run_device call over power float32 [S, nb, N] -> (stations STATION_DTYPE [S, max_stations], counts int32 [S, 2], chan float32
    [S, C] or None); every output buffer starts as 0xff bytes"""
    import torch
    dev = torch.device("cuda:0")
    S, nb, _ = power.shape
    d_p = torch.from_numpy(np.array(power)).to(dev)
    d_st = torch.full((S, scan.cfg.max_stations * 32), 255, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((S, 2), -1, dtype=torch.int32, device=dev)
    d_ch = torch.full((S, scan.n_candidates), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    scan.run_device(d_p, nb, d_st, d_cnt, d_ch if want_chan else None, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    scan.sync()
    ch = d_ch.cpu().numpy()
    if not want_chan:
        assert np.all(ch == -7.0), "d_chan = NULL and yet written"
    return d_st.cpu().numpy().view(M.STATION_DTYPE).reshape(S, -1), d_cnt.cpu().numpy(), ch if want_chan else None


def same_bits(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", [c[0] for c in M.CASES])
def test_the_cases_against_the_model(R, name):
    cfg, power, want = case(name)
    scan = R.Scan(c_config(R, cfg), power.shape[0])
    assert scan.n_candidates == want[0]["plan"]["C"]
    st, cnt, ch = run_dev(scan, power)
    exact = 0
    for s, res in enumerate(want):
        M.assert_matches(res, st[s], cnt[s], ch[s], cfg, "%s, stream %d" % (name, s))
        exact += st[s].tobytes() == res["stations"].tobytes() and ch[s].tobytes() == res["chan"].tobytes()
    print("%s: found %s, %d of %d streams equal to the model bit for bit" % (name, [int(c[0]) for c in cnt], exact, len(want)))
    # d_chan = NULL: the same stations and counts, and nothing written through it
    st2, cnt2, _ = run_dev(scan, power, want_chan=False)
    assert same_bits((st, cnt), (st2, cnt2))
    scan.close()


def test_bit_equality_alone_among_others_on_a_callers_stream_and_through_the_host_form(R):
    import torch
    cfg, power, _ = case("n256 b3 s5 guard3")
    scan = R.Scan(c_config(R, cfg), 5)
    whole = run_dev(scan, power)
    one = R.Scan(c_config(R, cfg), 1)
    for s in range(5):
        alone = run_dev(one, power[s:s + 1])
        assert same_bits(alone, tuple(x[s:s + 1] for x in whole)), s
    st = torch.cuda.Stream()
    assert same_bits(run_dev(scan, power, stream=st), whole)
    assert same_bits(run_dev(scan, power), whole)                        # back on the own stream: no state, nothing to hand over
    host = scan.run_host(power, power.shape[1])
    assert same_bits((host[0].view(M.STATION_DTYPE), host[1], host[2]), whole)
    h2 = scan.run_host(power[:, :1], 1, chan=False)                      # fewer blocks through the same staging; chan not asked for
    assert h2[2] is None and same_bits((h2[0].view(M.STATION_DTYPE), h2[1]), run_dev(scan, power[:, :1])[:2])
    one.close()
    scan.close()


def test_a_captured_graph_replays_to_the_bits_of_the_plain_launch(R):
    """One torch stream, one kernel: captured once - right after a launch on the object's own stream, which needs no hand-over - and replayed twice
    with the input refilled in between; each replay equals the plain launch on the same input."""
    import torch
    cfg, power, _ = case("n64 b3 s5 guard1 sep3")
    other = np.ascontiguousarray(power[::-1])                            # the streams in reverse order: another launch's input
    scan = R.Scan(c_config(R, cfg), 5)
    want = [run_dev(scan, p) for p in (power, other)]
    dev = torch.device("cuda:0")
    d_p = torch.zeros(power.shape, dtype=torch.float32, device=dev)
    d_st = torch.full((5, cfg["max_stations"] * 32), 255, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((5, 2), -1, dtype=torch.int32, device=dev)
    d_ch = torch.full((5, scan.n_candidates), -7.0, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    scan.run_device(d_p, power.shape[1], d_st, d_cnt, d_ch)              # the own stream; the capture below is on another
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        scan.run_device(d_p, power.shape[1], d_st, d_cnt, d_ch, hip_stream=st.cuda_stream)
    scan.sync()
    for r, p in enumerate((power, other)):
        d_p.copy_(torch.from_numpy(np.array(p)))
        d_st.fill_(255)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (d_st.cpu().numpy().view(M.STATION_DTYPE).reshape(5, -1), d_cnt.cpu().numpy(), d_ch.cpu().numpy())
        assert same_bits(got, want[r]), r
    scan.close()


def test_argument_checks_on_the_device(R):
    import torch
    cfg, power, _ = case("n64 b1 s1")
    scan = R.Scan(c_config(R, cfg), 1)
    dev = torch.device("cuda:0")
    d_p = torch.zeros(64 + 4, dtype=torch.float32, device=dev)
    d_st = torch.zeros(cfg["max_stations"] * 32 + 16, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(8, dtype=torch.int32, device=dev)
    L, p = R.lib(), lambda t, off=0: C.c_void_p(t.data_ptr() + off)     # noqa: E731
    for args in ((p(d_p), 0, p(d_st), p(d_cnt), None), (p(d_p), -1, p(d_st), p(d_cnt), None), (None, 1, p(d_st), p(d_cnt), None),
                 (p(d_p), 1, None, p(d_cnt), None), (p(d_p), 1, p(d_st), None, None), (p(d_p, 4), 1, p(d_st), p(d_cnt), None),
                 (p(d_p), 1, p(d_st, 8), p(d_cnt), None), (p(d_p), 1, p(d_st), p(d_cnt, 4), None), (p(d_p), 1, p(d_st), p(d_cnt), p(d_p, 4))):
        assert L.fmd_scan_run_device(scan._h, args[0], args[1], args[2], args[3], args[4], None) == FMD_E_ARG and L.fmd_last_error(), args
    with pytest.raises(R.FmdError):
        R.Scan(c_config(R, cfg), 0)
    scan.close()


E2E_STEP, E2E_TUNER_BW, E2E_TAPS = 1000, 120000, 64      # as tests/test_scan_cpu.py, test_end_to_end_in_the_models


def test_end_to_end_spectrum_scan_tuner_spectrum_scan(R):
    """The capture of scan_model.capture_bytes (three FM carriers, noise, a DC offset) through fmd_batch_spectrum_device into the scan (N = 256,
    dc_guard 2): the offsets are the planted ones, strongest first.  fmd_tuner_shift of the first station feeds the tuner (offset_tuning, bw 120 k);
    its output through spectrum and scan again has its first station at offset 0.  All on one stream, nothing copied to the host in between."""
    import torch
    dev = torch.device("cuda:0")
    bl, nb = M.CAPTURE_BLOCK_LEN, M.CAPTURE_BLOCKS
    cfg = M.capture_config(256, 2)
    b = R.BatchDemod(R.wbfm_config(rate_in=M.CAPTURE_RATE // 8, rate_out2=48000, mode=2, block_len=bl, math=R.MATH_FAST, offset_tuning=True), 1)
    scan = R.Scan(c_config(R, cfg), 1)
    by_batch = b.scan(256, 100000, 100000, max_stations=16)              # the batch's own: dc_guard 0
    assert by_batch.n_candidates == scan.n_candidates == 21 and by_batch.cfg.rate == M.CAPTURE_RATE
    tc = R.FmdTunerConfig(M.CAPTURE_RATE, E2E_STEP, E2E_TUNER_BW, E2E_TAPS, bl, 0)
    tun = R.Tuner(tc, 1, 1)
    d_iq = torch.from_numpy(np.array(M.capture_bytes()).reshape(1, nb, bl)).to(dev)
    d_out = torch.zeros((1, nb, bl), dtype=torch.uint8, device=dev)
    power = torch.zeros((1, nb, 256), dtype=torch.float32, device=dev)
    d_st = torch.full((3, 16 * 32), 255, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((3, 4), -1, dtype=torch.int32, device=dev)          # (rows of 16 bytes: the alignment of d_counts)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    b.spectrum_device(d_iq, nb, 256, power, hip_stream=st.cuda_stream)
    scan.run_device(power, nb, d_st[0], d_cnt[0], hip_stream=st.cuda_stream)
    by_batch.run_device(power, nb, d_st[1], d_cnt[1], hip_stream=st.cuda_stream)
    st.synchronize()
    first = d_st[0].cpu().numpy().view(M.STATION_DTYPE)
    n = int(d_cnt[0, 1])
    assert [int(x) for x in first["offset_hz"][:n]] == [f for f, _ in M.CAPTURE_CARRIERS], first[:n]
    assert np.all(np.abs(first["centroid_hz"][:n] - first["offset_hz"][:n]) < 5000)
    unguarded = d_st[1].cpu().numpy().view(M.STATION_DTYPE)[:int(d_cnt[1, 1])]
    assert sorted(int(x) for x in unguarded["offset_hz"]) == sorted([0] + [f for f, _ in M.CAPTURE_CARRIERS])     # without the guard: the DC spike too
    tun.set_channel(0, 0, R.tuner_shift(tc, int(first["offset_hz"][0]), True), 1.0)
    tun.run_device(d_iq, nb, d_out, hip_stream=st.cuda_stream)
    b.spectrum_device(d_out, nb, 256, power, hip_stream=st.cuda_stream)
    scan.run_device(power, nb, d_st[2], d_cnt[2], hip_stream=st.cuda_stream)
    st.synchronize()
    second = d_st[2].cpu().numpy().view(M.STATION_DTYPE)
    assert int(d_cnt[2, 0]) >= 1 and second["offset_hz"][0] == 0 and second["candidate"][0] == 10, second[:int(d_cnt[2, 1])]
    for o in (tun, scan, by_batch):
        o.sync()
        o.close()
    b.close()
