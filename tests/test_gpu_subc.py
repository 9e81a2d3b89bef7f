"""The MPX subcarrier receiver on the device (fmd_subc_*; include/fmdemod_mi355x.h, "MPX subcarrier receiver"; csrc/subcarrier.inc).

Every result is held to subc_model.subc_bound against the float64 model of the same v and taps - a bound on structure (a wrong tap, a lost or
doubled history sample, a phase slip exceed it by orders of magnitude: tests/test_subc_cpu.py), not a precision contest - and to bit equality
wherever the header says the result depends on the stream's v alone: the split into calls, the number of streams, the stream used, the host
form, a captured graph.  The device gets the very taps the model uses.

Shapes: the smallest at which the kernel can go wrong.  (300 k, 19 kHz, T 256, D 16, M 256): the history is the whole block before and
Pd = 300 does not divide M, so the phase is non-zero at block starts; (192 k, 57 kHz, 16, 4, 512): the shortest filter, several outputs per
thread; (300 k, 57 kHz, 128, 32, 512): fewer outputs than threads; (240 k, 57 kHz, 96, 8, 1024).  M = 4608 and 8192 add blocks of more than one
chunk (4096 samples), ragged and whole."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subc_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

#          rate    fc     bw    T    D   M
SHAPES = [(300000, 19000, 500, 256, 16, 256), (192000, 57000, 2400, 16, 4, 512), (300000, 57000, 2400, 128, 32, 512), (240000, 57000, 2400, 96, 8, 1024)]
CHUNKED = [(300000, 57000, 2400, 128, 16, 4608), (300000, 19000, 500, 64, 4, 8192)]
WORST = {"share": 0.0}        # the largest share of the bound the kernel has used so far in this session (printed by every model test)


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@functools.lru_cache(maxsize=None)
def taps_of(rate, bw, T):
    t = SM.design(rate, bw, T).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def input_of(kind, rate, fc, S, n):
    """float32 [S, n], read-only; every stream its own values so that a stream mix-up shows"""
    if kind == "lcg":
        a = np.stack([SM.lcg_floats(n, 7 + 13 * s) for s in range(S)])
    elif kind == "tone":
        a = np.stack([SM.tone(n, rate, fc, amp=0.3 + 0.1 * s, phi=0.7 + s) for s in range(S)])
    elif kind == "zeros":
        a = np.zeros((S, n), dtype=np.float32)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


def make(R, shape, S, taps=None):
    rate, fc, bw, T, D, M = shape
    return R.Subcarrier(R.FmdSubcConfig(rate, fc, bw, T, D, M), S, taps=taps_of(rate, bw, T) if taps is None else taps)


def run_dev(sub, v, stream=None):
    """one fmd_subc_run_device call over v float32 [S, nb, M] -> complex64 [S, nb, M / D] (numpy); stream: a torch stream or None"""
    import torch
    dev = torch.device("cuda:0")
    S, nb = v.shape[0], v.shape[1]
    d_v = torch.from_numpy(np.array(v, dtype=np.float32).reshape(-1)).to(dev)
    d_z = torch.full((S, nb, sub.out_per_block, 2), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sub.run_device(d_v, nb, d_z, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    sub.sync()
    return d_z.cpu().numpy().view(np.complex64)[..., 0]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bound(got, v, shape, what, hist=None, phase=0, taps=None):
    """got complex64 [S, nb, M / D] of v [S, nb, M] from the state (phase, hist [S, T]) against the float64 model, output by output"""
    rate, fc, bw, T, D, M = shape
    taps = taps_of(rate, bw, T) if taps is None else taps
    assert got.dtype == np.complex64 and got.shape == (v.shape[0], v.shape[1], M // D), (got.shape, v.shape)
    assert np.isfinite(got.view(np.float32)).all(), what
    for s in range(v.shape[0]):
        vs = v[s].reshape(-1)
        h = None if hist is None else hist[s]
        z64, _ = SM.subc_f64(vs, taps, rate, fc, D, phase, h)
        share = SM.bound_share(got[s].reshape(-1), z64, SM.subc_bound(vs, taps, D, h))
        WORST["share"] = max(WORST["share"], share)
        print("%s stream %d: share of the bound %.4f (largest so far %.4f)" % (what, s, share, WORST["share"]))
        assert share < 1, (what, s, share)


# ---- 1. against the float64 model --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("shape", SHAPES + CHUNKED)
def test_subcarrier_matches_the_model(R, shape, S, nb):
    rate, fc, bw, T, D, M = shape
    sub = make(R, shape, S)
    assert sub.out_per_block == M // D
    for kind in ("lcg", "tone", "zeros"):
        v = input_of(kind, rate, fc, S, nb * M).reshape(S, nb, M)
        sub.reset()
        got = run_dev(sub, v)
        assert_bound(got, v, shape, "%s T %d D %d M %d S %d nb %d" % (kind, T, D, M, S, nb))
        if kind == "zeros":
            assert not got.view(np.uint32).any()                       # exactly zero, +0
        if kind == "tone" and nb * M >= 8 * T and T >= 64:             # (16 taps leave the image at 2 fc in)
            for s in range(S):                                          # the settled tone reads A e^(i phi)
                z = got[s].reshape(-1)[T // D + 1:]
                assert np.abs(z - (0.3 + 0.1 * s) * np.exp(1j * (0.7 + s))).max() <= 2e-4 * (0.3 + 0.1 * s)
    sub.close()


@pytest.mark.parametrize("split", ["same launch", "next call"])
@pytest.mark.parametrize("shape", SHAPES)
def test_an_impulse_on_a_blocks_last_sample_appears_in_the_next_block_scaled_by_the_taps(R, shape, split):
    """v = a on the last sample of block 0 (sample count M - 1), nothing else: output m of block 1 is a c[(M - 1) mod Pd] h[mD + D] - through the
    block before it in the same launch, or through the carried state in the next call"""
    rate, fc, bw, T, D, M = shape
    S = 2
    amp = np.array([1.0, -2.5])
    v = np.zeros((S, 2, M), dtype=np.float32)
    v[:, 0, M - 1] = amp
    sub = make(R, shape, S)
    got = run_dev(sub, v) if split == "same launch" else np.concatenate([run_dev(sub, v[:, 0:1]), run_dev(sub, v[:, 1:2])], axis=1)
    sub.close()
    assert_bound(got, v, shape, "impulse, %s, T %d D %d" % (split, T, D))
    taps = taps_of(rate, bw, T).astype(np.float64)
    c = SM.carrier_exact(rate, fc, M - 1, 1)[0]
    k = np.arange(M // D) * D + D
    want = np.where(k < T, taps[np.minimum(k, T - 1)], 0.0)
    for s in range(S):
        z1 = got[s, 1].astype(np.complex128)
        assert np.abs(z1 - amp[s] * c * want).max() <= 4 * 2.0 ** -24 * 2 * abs(amp[s]) * np.abs(taps).max()
        assert not got[s, 1][k >= T].view(np.uint32).any()             # past the filter's reach: exactly zero
        assert np.count_nonzero(got[s, 1]) == np.count_nonzero(want)
        assert not got[s, 0, :-1].view(np.uint32).any() and got[s, 0, -1] != 0      # block 0: the last output alone, through h[0]


# ---- 2. bit equality: the result depends on the stream's v alone --------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES + CHUNKED[:1])
def test_split_invariance(R, shape):
    """6 blocks in one call = 1 + 2 + 3 across calls = six single calls, bit for bit; stream s of a 3-stream object = a 1-stream object fed the
    same v"""
    rate, fc, bw, T, D, M = shape
    S, nb = 3, 6
    v = input_of("lcg", rate, fc, S, nb * M).reshape(S, nb, M)
    sub = make(R, shape, S)
    whole = run_dev(sub, v)
    assert_bound(whole, v, shape, "split invariance T %d D %d M %d" % (T, D, M))
    sub.reset()
    a = np.concatenate([run_dev(sub, v[:, 0:1]), run_dev(sub, v[:, 1:3]), run_dev(sub, v[:, 3:6])], axis=1)
    assert same_bits(a, whole)
    sub.reset()
    b = np.concatenate([run_dev(sub, v[:, k:k + 1]) for k in range(nb)], axis=1)
    assert same_bits(b, whole)
    sub.close()
    for s in range(S):
        one = make(R, shape, 1)
        assert same_bits(run_dev(one, v[s:s + 1]), whole[s:s + 1]), s
        one.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_state_hand_over(R, shape):
    """get_state after k blocks is the model's (phase, last T samples); set_state into a fresh object continues bit-equal; reset zeroes it"""
    rate, fc, bw, T, D, M = shape
    S, nb, k = 2, 5, 3
    v = input_of("lcg", rate, fc, S, nb * M).reshape(S, nb, M)
    sub = make(R, shape, S)
    whole = run_dev(sub, v)
    sub.reset()
    first = run_dev(sub, v[:, :k])
    states = [sub.get_state(s) for s in range(S)]
    for s in range(S):
        _, (phase, hist) = SM.subc_f64(v[s, :k].reshape(-1), taps_of(rate, bw, T), rate, fc, D)
        assert states[s].phase == phase == (k * M) % SM.period(rate, fc)
        assert np.array_equal(np.array(states[s].hist[:T], dtype=np.float32).view(np.uint32), hist.view(np.uint32))
    fresh = make(R, shape, S)
    for s in range(S):
        fresh.set_state(s, states[S - 1 - s])                           # crossed over: stream s continues stream S-1-s
    rest = run_dev(fresh, v[::-1, k:])[::-1]
    assert same_bits(np.concatenate([first, rest], axis=1), whole)
    # out of range: refused, nothing changed
    bad = R.FmdSubcState()
    bad.phase = SM.period(rate, fc)
    assert R.lib().fmd_subc_set_state(fresh._h, 0, C.byref(bad)) == -1
    fresh.reset()
    for s in range(S):
        assert not any(bytes(fresh.get_state(s)))
    assert same_bits(run_dev(fresh, v), whole)
    fresh.close()
    sub.close()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], CHUNKED[0]])
def test_the_host_form_equals_the_device_form(R, shape):
    rate, fc, bw, T, D, M = shape
    S, nb = 3, 4
    v = input_of("lcg", rate, fc, S, nb * M).reshape(S, nb, M)
    a, b = make(R, shape, S), make(R, shape, S)
    dev = np.concatenate([run_dev(a, v[:, :1]), run_dev(a, v[:, 1:])], axis=1)
    host = np.concatenate([b.run_host(v[:, :3], 3), b.run_host(v[:, 3:], 1)], axis=1)      # (the staging shrinks: kept)
    assert same_bits(host, dev)
    # the two forms interleave on one object
    a.reset()
    mixed = np.concatenate([a.run_host(v[:, :2], 2), run_dev(a, v[:, 2:])], axis=1)
    assert same_bits(mixed, dev)
    a.close()
    b.close()


def test_a_launch_on_a_callers_stream_then_one_on_the_objects_own_stream(R):
    """The second launch reads the state the first one writes: the library orders them with an event.  The first is long (32 streams x 48 blocks of
    8192), the second follows at once on the other stream; then back to the caller's stream.  Bit-equal to one stream throughout."""
    import torch
    shape = (300000, 19000, 500, 256, 16, 8192)
    rate, fc, bw, T, D, M = shape
    S, nb = 32, 50
    rng = np.random.default_rng(11)
    v = (rng.random((S, nb, M), dtype=np.float32) * 2 - 1) * np.float32(np.pi)
    dev = torch.device("cuda:0")
    d_v = torch.from_numpy(v.reshape(-1)).to(dev).reshape(S, nb, M)
    parts = [d_v[:, :48].contiguous(), d_v[:, 48:49].contiguous(), d_v[:, 49:].contiguous()]
    ref, two = make(R, shape, S), make(R, shape, S)
    z_ref = [torch.zeros((S, p.shape[1], M // D, 2), dtype=torch.float32, device=dev) for p in parts]
    z_two = [torch.zeros_like(z) for z in z_ref]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for p, z in zip(parts, z_ref):
        ref.run_device(p, p.shape[1], z)
    ref.sync()
    two.run_device(parts[0], 48, z_two[0], hip_stream=st.cuda_stream)
    two.run_device(parts[1], 1, z_two[1])
    two.run_device(parts[2], 1, z_two[2], hip_stream=st.cuda_stream)
    two.sync()
    st.synchronize()
    for a, b in zip(z_ref, z_two):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert bytes(ref.get_state(1)) == bytes(two.get_state(1))
    got = np.concatenate([z.cpu().numpy().view(np.complex64)[..., 0] for z in z_two], axis=1)
    assert_bound(got[:1, :2], v[:1, :2], shape, "two streams")
    ref.close()
    two.close()


def test_a_captured_graph_replays_to_the_bits_of_the_eager_launch(R):
    """One torch stream, no branches: {receiver kernel, state kernel} of a 2-block launch captured once, replayed three times with v refilled in
    between.  The state advances in place, so replay r continues replay r - 1: bit-equal to three eager launches on a fresh object.  A launch
    whose stream differs from the previous launch's is refused inside a capture (FMD_E_STATE) and leaves the capture valid."""
    import torch
    shape = SHAPES[0]
    rate, fc, bw, T, D, M = shape
    S, nb, reps = 3, 2, 3
    v = input_of("lcg", rate, fc, S, reps * nb * M).reshape(S, reps, nb, M)
    dev = torch.device("cuda:0")
    eager, graphed = make(R, shape, S), make(R, shape, S)
    want = [run_dev(eager, v[:, r]) for r in range(reps)]
    d_v = torch.zeros((S, nb, M), dtype=torch.float32, device=dev)
    d_z = torch.zeros((S, nb, M // D, 2), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        graphed.run_device(d_v, nb, d_z, hip_stream=st.cuda_stream)
    for r in range(reps):
        d_v.copy_(torch.from_numpy(np.array(v[:, r])).to(dev))
        d_z.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(d_z.cpu().numpy().view(np.complex64)[..., 0], want[r]), r
    assert [bytes(graphed.get_state(s)) for s in range(S)] == [bytes(eager.get_state(s)) for s in range(S)]
    # the previous launch on another stream: no event hand-over inside a capture
    graphed.run_device(d_v, nb, d_z)                  # the object's own stream
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        rc = R.lib().fmd_subc_run_device(graphed._h, C.c_void_p(d_v.data_ptr()), nb, C.c_void_p(d_z.data_ptr()), C.c_void_p(st.cuda_stream))
        msg = R.lib().fmd_last_error().decode()
        d_z.fill_(3.0)
    assert rc == -6 and "fmd_subc_sync" in msg, (rc, msg)
    graphed.sync()
    g2.replay()
    torch.cuda.synchronize()
    assert bool((d_z == 3.0).all())
    eager.close()
    graphed.close()


def test_argument_checks_on_the_device(R):
    import torch
    shape = SHAPES[1]
    sub = make(R, shape, 1)
    L = R.lib()
    dev = torch.device("cuda:0")
    d_v = torch.zeros(2 * 512 + 4, dtype=torch.float32, device=dev)
    d_z = torch.zeros(2 * 256 + 4, dtype=torch.float32, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.fmd_subc_run_device(sub._h, p(d_v, 4), 1, p(d_z), None) == -1 and b"16-byte" in L.fmd_last_error()
    assert L.fmd_subc_run_device(sub._h, p(d_v), 1, p(d_z, 8), None) == -1
    assert L.fmd_subc_run_device(sub._h, p(d_v), -1, p(d_z), None) == -1
    assert L.fmd_subc_run_device(sub._h, p(d_v), 0, p(d_z), None) == 0
    assert L.fmd_subc_run_device(sub._h, p(d_v), 1 << 23, p(d_z), None) == -1 and b"too large" in L.fmd_last_error()
    st = R.FmdSubcState()
    assert L.fmd_subc_get_state(sub._h, 1, C.byref(st)) == -1 and L.fmd_subc_get_state(sub._h, 0, C.byref(st)) == 0
    sub.close()


# ---- 3. end to end with the demodulator ------------------------------------------------------------------------------------------------------

def test_the_pilot_meter_on_the_demodulators_v_tap(R):
    """A FMD_MATH_FAST stereo batch at 300 k, block_len 8192, 2 streams x 6 blocks of the DDS multiplex, the pilot on for stream 0 and off for
    stream 1: run_device(debug={"v": ...}), then Batch.subcarrier(19000, 500) straight on the tap's buffer.  z within the bound of the model
    applied to the downloaded v; mean |z| past the filter's first 16 outputs 0.150 .. 0.160 with the pilot and below 0.005 without; and the PCM
    is that of the same launch without the subcarrier call."""
    import torch
    from oracle import dds_bytes
    bl, nb, S = 8192, 6, 2
    M = bl // 16
    dev = torch.device("cuda:0")
    iq_np = np.stack([dds_bytes(bl * nb, stereo=1), dds_bytes(bl * nb, stereo=0)])
    iq = torch.from_numpy(iq_np.reshape(-1)).to(dev)
    cfg = R.wbfm_config(rate_in=300000, rate_out2=48000, mode=2, block_len=bl, math=R.MATH_FAST)
    out = []
    for with_subc in (True, False):
        b = R.BatchDemod(cfg, S)
        pcm = torch.zeros(S * nb * b.pcm_stride, dtype=torch.int16, device=dev)
        lens = torch.zeros(S * nb, dtype=torch.int32, device=dev)
        v = torch.zeros((S, nb, M), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        b.run_device(iq, nb, pcm, lens, debug={"v": v})
        b.sync()                                       # the subcarrier object launches on a stream of its own: v must be complete
        if with_subc:
            sub = b.subcarrier(19000, 500)
            assert (sub.cfg.rate_in, sub.cfg.block_samples, sub.cfg.n_taps, sub.cfg.decim, sub.n_streams, sub.out_per_block) == (300000, M, 128, 16, S, M // 16)
            z = torch.zeros((S, nb, M // 16, 2), dtype=torch.float32, device=dev)
            sub.run_device(v, nb, z)
            sub.sync()
            sub.close()
        torch.cuda.synchronize()
        out.append((pcm.cpu().numpy(), lens.cpu().numpy(), v.cpu().numpy()))
        b.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and same_bits(out[0][2], out[1][2])
    assert out[0][1].min() > 0
    got = z.cpu().numpy().view(np.complex64)[..., 0]
    v_np = out[0][2]
    # the default taps of the convenience constructor are fmd_subc_design's
    shape = (300000, 19000, 500, 128, 16, M)
    assert_bound(got, v_np, shape, "pilot meter on the v tap", taps=R.subc_design(R.FmdSubcConfig(*shape)))
    level = np.abs(got.reshape(S, -1)[:, 16:]).mean(axis=1)
    print("mean |z|: pilot on %.4f, off %.4f" % (level[0], level[1]))
    assert 0.150 <= level[0] <= 0.160
    assert level[1] < 0.005
