"""The channel tuner on the device (fmd_tuner_*; include/fmdemod_mi355x.h, "Channel tuner"; csrc/tuner.inc).

The bytes are held three ways against tests/tuner_model.py:
  1. out equals the quantiser applied to the device's own d_y - every output, exact;
  2. d_y is within tuner_model.tuner_bound of the float64 model - every output;
  3. out equals the float64 model's codes wherever the model's pre-rounding value lies further than G bound + 2^-16 from a boundary; elsewhere the
     two differ by at most 1.  The exempt set of every case is at most 1 % of it: tests/test_tuner_cpu.py asserts that from the float64 model alone,
     so the cases (tuner_model.MODEL_CASES) are fixed without a device.
and to bit equality wherever the header says the result depends on the source's bytes and the channel alone: the split into calls, the number of
channels, the stream used, the host form, a captured graph.  The device gets the very taps the model uses.

Shapes: the smallest that reach each path.  block_len 64 with T = 16 (L = 32: the history is half the block); 512 (a block shorter than a chunk);
2 (4096 + 24) (a whole chunk and a ragged one); 16384 (two whole chunks); P = 2400 (does not divide L: the count is non-zero at block starts), 4 and
4096; T = 16 and 64; 2 sources x 5 channels with a mixed source map, every source its own bytes; 3 blocks."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_model as SP  # noqa: E402
import tuner_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

FMD_E_ARG, FMD_E_STATE = -1, -6
WORST = {"share": 0.0}        # the largest share of the bound the kernel has used so far in this session (printed by every model test)
IMPULSE16 = np.array([1.0] + [0.0] * 15, dtype=np.float32)
RAGGED = 2 * (4096 + 24)


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@functools.lru_cache(maxsize=None)
def input_of(kind, n_bytes, source):
    a = TM.all_values_bytes(n_bytes) if kind == "all" else TM.dc_bytes(n_bytes) if kind == "dc" else TM.case_input(kind, n_bytes, source)
    if kind == "all" and source:
        a = a[::-1].copy()                              # (every source its own bytes)
    a.setflags(write=False)
    return a


def sources(kind, bl, nb, n_src=TM.N_SOURCES):
    """uint8 [n_src, nb, bl]"""
    return np.stack([input_of(kind, bl * nb, s).reshape(nb, bl) for s in range(n_src)])


def make(R, T, P, bl, n_src, chans, taps=None):
    """a Tuner at the case's rate with the channels [(source, shift, gain)] set"""
    rate = TM.case_rate(P)
    t = R.Tuner(R.FmdTunerConfig(rate, rate // P, rate // 24, T, bl, 0), n_src, len(chans), taps=TM.case_taps(T, P) if taps is None else taps)
    for c, (src, sh, g) in enumerate(chans):
        t.set_channel(c, src, sh, g)
    return t


def run_dev(t, iq, stream=None, want_y=True):
    """one fmd_tuner_run_device call over iq uint8 [S, nb, bl] -> (out uint8 [C, nb, bl], y complex64 [C, nb, L] or None); stream: a torch stream or None"""
    import torch
    dev = torch.device("cuda:0")
    nb, bl = iq.shape[1], iq.shape[2]
    d_iq = torch.from_numpy(np.ascontiguousarray(iq).reshape(-1)).to(dev)
    d_out = torch.full((t.n_channels, nb, bl), 77, dtype=torch.uint8, device=dev)
    d_y = torch.full((t.n_channels, nb, bl // 2, 2), -7.0, dtype=torch.float32, device=dev) if want_y else None
    torch.cuda.synchronize()
    t.run_device(d_iq, nb, d_out, d_y, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    t.sync()
    return d_out.cpu().numpy(), (d_y.cpu().numpy().view(np.complex64)[..., 0] if want_y else None)


def check_rules(out, y, iq, chans, taps, P, what, rule3=True, states=None):
    """out uint8 [C, nb, bl] and y complex64 [C, nb, L] of iq uint8 [S, nb, bl] against the models, channel by channel, from the per-source states
    [(count, hist)] (None: after a reset).  Returns (exempt, all) counts of rule 3."""
    n_ex = n_all = 0
    assert out.dtype == np.uint8 and y.dtype == np.complex64 and np.isfinite(y.view(np.float32)).all(), what
    for c, (src, sh, g) in enumerate(chans):
        stream = iq[src].reshape(-1)
        count, hist = (0, None) if states is None else states[src]
        y64, _ = TM.run_blocks(TM.tuner_f64, stream, iq.shape[2], taps, P, sh, count, hist)
        bound = TM.tuner_bound(stream, taps, hist)
        got, yc = out[c].reshape(-1), y[c].reshape(-1)
        # 1. the bytes are the quantiser of the device's own y: exact
        assert np.array_equal(got, TM.quantise_f32(yc, g)), (what, c, "rule 1")
        # 2. y within the bound of the float64 model
        share = TM.bound_share(yc, y64, bound)
        WORST["share"] = max(WORST["share"], share)
        print("%s channel %d (source %d shift %d gain %g): share of the bound %.4f (largest so far %.4f)" % (what, c, src, sh, g, share, WORST["share"]))
        assert share < 1, (what, c, "rule 2", share)
        # 3. the bytes are the float64 model's away from the boundaries, within 1 at them
        if rule3:
            codes, v = TM.codes_f64(y64, g)
            ex = TM.exempt(v, bound, g)
            d = np.abs(got.astype(np.int32) - codes.astype(np.int32))
            assert d[~ex].max() == 0 and d.max() <= 1, (what, c, "rule 3", int(d[~ex].max()), int(d.max()))
            n_ex += int(ex.sum())
            n_all += ex.size
    return n_ex, n_all


# ---- 1. against the models -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TM.MODEL_CASES, ids=[c[0] for c in TM.MODEL_CASES])
def test_tuner_matches_the_model(R, case):
    name, kind, T, P, shift, gain, bl, nb = case
    chans = TM.case_channels(P, shift, gain)
    iq = sources(kind, bl, nb)
    t = make(R, T, P, bl, TM.N_SOURCES, chans)
    out, y = run_dev(t, iq)
    t.close()
    n_ex, n_all = check_rules(out, y, iq, chans, TM.case_taps(T, P), P, name)
    print("%s: exempt %d of %d = %.3f %%" % (name, n_ex, n_all, 100.0 * n_ex / n_all))
    assert n_ex <= 0.01 * n_all
    if kind == "lcg" and gain == 8.0:
        assert (out == 0).any() and (out == 255).any()              # the clamps are reached (and match the model: rule 3)


@pytest.mark.parametrize("kind,shift", [("quiet", 0), ("quiet", -700), ("dc", TM.EMPTY_PASSBAND_SHIFT), ("dc", 0)])
def test_quiet_input_and_an_empty_passband_pass_rules_1_and_2(R, kind, shift):
    """Bytes in {127, 128}, and a capture whose only content is moved out of the passband: the output sits on the tie at 127.5, so rule 3 does not
    apply (tests/test_tuner_cpu.py); the codes are 127 / 128 (dc at shift 0: the DC term itself, in band)"""
    T, P, bl, nb = 64, 2400, 512, 3
    chans = [(0, shift, 1.0), (1, shift, 8.0)]
    iq = sources(kind, bl, nb)
    t = make(R, T, P, bl, 2, chans)
    out, y = run_dev(t, iq)
    t.close()
    check_rules(out, y, iq, chans, TM.case_taps(T, P), P, "%s shift %d" % (kind, shift), rule3=False)
    if not (kind == "dc" and shift == 0):
        settled = out[0].reshape(-1)[2 * T:]
        assert set(np.unique(settled)) <= {127, 128}


# ---- 2. exact cases ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [4, 2400, 4096])
@pytest.mark.parametrize("bl", [64, 512, RAGGED])
def test_identity_and_quarter_turn(R, bl, P):
    """h = (1, 0, ...), gain 1.  Shift 0: the output bytes are the input bytes.  Shift +P/4: the reference's rotate_90 byte pattern
    (I, Q), (255 - Q, I), (255 - I, 255 - Q), (Q, 255 - I).  Over an input that holds all 256 values in both components."""
    nb = 3
    iq = sources("all", bl, nb)
    assert set(iq[0, :, 0::2].reshape(-1)) == set(range(256)) or bl == 64
    chans = [(0, 0, 1.0), (1, 0, 1.0), (0, P // 4, 1.0), (1, P // 4, 1.0), (1, -3 * P // 4, 1.0)]
    t = make(R, 16, P, bl, 2, chans, taps=IMPULSE16)
    out, y = run_dev(t, iq)
    t.close()
    for c, (src, sh, _) in enumerate(chans):
        want = iq[src].reshape(-1) if sh == 0 else TM.rotate_90_bytes(iq[src].reshape(-1))
        assert np.array_equal(out[c].reshape(-1), want), (c, src, sh)
    check_rules(out, y, iq, chans, IMPULSE16, P, "identity / quarter turn P %d block_len %d" % (P, bl))


def batch_pcm(R, d_iq, n_streams, nb, bl, math, offset_tuning):
    """the PCM of d_iq (a device tensor u8 [n_streams, nb, bl]) through a 300 k stereo batch: [per stream: int16 concatenated over the blocks]"""
    import torch
    cfg = R.wbfm_config(rate_in=300000, rate_out2=48000, mode=2, block_len=bl, math=math, offset_tuning=offset_tuning)
    b = R.BatchDemod(cfg, n_streams)
    pcm = torch.zeros(n_streams * nb * b.pcm_stride, dtype=torch.int16, device=d_iq.device)
    lens = torch.zeros(n_streams * nb, dtype=torch.int32, device=d_iq.device)
    torch.cuda.synchronize()
    b.run_device(d_iq, nb, pcm, lens)
    b.sync()
    p, n = pcm.cpu().numpy().reshape(n_streams, nb, b.pcm_stride), lens.cpu().numpy().reshape(n_streams, nb)
    b.close()
    assert n.min() > 0
    return [np.concatenate([p[s, k, :n[s, k]] for k in range(nb)]) for s in range(n_streams)]


def test_the_quarter_turn_feeds_an_offset_tuning_batch_the_pcm_of_the_original(R):
    """The tuner's quarter turn is the chain's own rotate_90: its bytes through a batch with offset_tuning = 1 give the PCM of the original bytes
    through a batch with offset_tuning = 0 - bit for bit with FMD_MATH_EXACT, within +-1 with FMD_MATH_FAST (whether the fast family is equal too
    is printed: DESIGN.md section 5e)."""
    import torch
    from oracle import dds_bytes
    bl, nb, P = 16384, 3, 2400
    dev = torch.device("cuda:0")
    iq = dds_bytes(bl * nb).reshape(1, nb, bl)
    t = make(R, 16, P, bl, 1, [(0, P // 4, 1.0)], taps=IMPULSE16)
    d_iq = torch.from_numpy(iq.reshape(-1)).to(dev).reshape(1, nb, bl)
    d_out = torch.zeros((1, nb, bl), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t.run_device(d_iq, nb, d_out)
    t.sync()
    t.close()
    assert np.array_equal(d_out.cpu().numpy().reshape(-1), TM.rotate_90_bytes(iq.reshape(-1)))
    for math, tol in ((R.MATH_EXACT, 0), (R.MATH_FAST, 1)):
        turned = batch_pcm(R, d_out, 1, nb, bl, math, True)[0]
        plain = batch_pcm(R, d_iq, 1, nb, bl, math, False)[0]
        assert turned.size == plain.size
        diff = int(np.abs(turned.astype(np.int32) - plain.astype(np.int32)).max())
        print("math %d: quarter turn + offset_tuning against the plain chain: largest PCM difference %d LSB over %d values" % (math, diff, plain.size))
        assert diff <= tol


def test_hand_in_to_the_batch_and_the_spectrum_without_a_copy(R):
    """The oracle's DDS multiplex moved by +300 kHz and requantised; BatchDemod.tuner (default taps, bw 800 kHz: the station comes back to -fs/4)
    with shift -300 tunes it back.  Its d_out goes straight into fmd_batch_run_device and fmd_batch_spectrum_device: the spectrum peaks where the
    original's does (bin 197 of 256 in block 0), and the EXACT family's PCM of those device bytes equals the oracle's PCM of the same bytes."""
    import torch
    from oracle import OracleStream, dds_bytes
    bl, nb = 16384, 3
    dev = torch.device("cuda:0")
    kw = dict(rate_in=300000, rate_out2=48000, mode=2)
    orig = dds_bytes(bl * nb, amp=100)
    moved = TM.shifted_bytes(orig, 300000, 2400000)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, math=R.MATH_EXACT, **kw), 1)
    t = b.tuner(1000, 800000)
    assert (t.cfg.rate, t.cfg.step_hz, t.cfg.bw, t.cfg.n_taps, t.cfg.block_len, t.n_sources, t.n_channels) == (2400000, 1000, 800000, 64, bl, 1, 1)
    ch = t.get_channel(0)
    assert (ch.source, ch.shift, ch.gain) == (0, 0, 1.0)
    assert R.tuner_shift(t.cfg, 300000 - 600000, False) == -300            # the station now 300 kHz above -fs/4 goes back there
    t.set_channel(0, 0, -300, 1.0)
    d_iq = torch.from_numpy(moved).to(dev)
    d_out = torch.zeros((1, nb, bl), dtype=torch.uint8, device=dev)
    pcm = torch.zeros(nb * b.pcm_stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(nb, dtype=torch.int32, device=dev)
    power = torch.zeros((1, nb, 256), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    t.run_device(d_iq, nb, d_out, hip_stream=st.cuda_stream)               # one stream: tuner, then the consumers of its bytes
    b.spectrum_device(d_out, nb, 256, power, window=R.WINDOW_RECT, hip_stream=st.cuda_stream)
    b.run_device(d_out, nb, pcm, lens, hip_stream=st.cuda_stream)
    st.synchronize()
    t.sync()
    b.sync()
    got_bytes = d_out.cpu().numpy().reshape(-1)
    peaks = [int(k) for k in power.cpu().numpy()[0].argmax(axis=1)]
    want_peaks = [int(np.argmax(SP.spectrum_f64(orig[k * bl:(k + 1) * bl], 256, SP.WINDOW_RECT))) for k in range(nb)]
    print("spectrum peaks of the tuned-back capture %s, of the original %s" % (peaks, want_peaks))
    assert peaks == want_peaks and peaks[0] == 197
    # the bytes are the model's (rule 3's sense) ...
    taps = R.tuner_design(t.cfg)
    y64, _ = TM.run_blocks(TM.tuner_f64, moved, bl, taps, 2400, -300)
    codes, v = TM.codes_f64(y64, 1.0)
    ex = TM.exempt(v, TM.tuner_bound(moved, taps), 1.0)
    d = np.abs(got_bytes.astype(np.int32) - codes.astype(np.int32))
    assert d[~ex].max() == 0 and d.max() <= 1
    # ... and their PCM is the oracle's PCM of the same bytes
    want, wlens = OracleStream(**kw).run(got_bytes, bl)
    n = lens.cpu().numpy()
    assert np.array_equal(n, wlens)
    p = pcm.cpu().numpy().reshape(nb, b.pcm_stride)
    assert np.array_equal(np.concatenate([p[k, :n[k]] for k in range(nb)]), want)
    t.close()
    b.close()


# ---- 3. bit equality: the result depends on the source's bytes and the channel alone ------------------------------------------------------------

@pytest.mark.parametrize("T,P,bl", [(64, 2400, RAGGED), (16, 2400, 64), (20, 2400, 64), (64, 4096, 512)])
def test_split_channel_count_stream_and_host_form_give_the_same_bytes(R, T, P, bl):
    """One call of 3 blocks = 3 calls of 1; channel c of 5 = a 1-channel tuner with that channel; the object's own stream = a caller's stream; the
    host form = the device form - bytes and y, bit for bit"""
    import torch
    nb = 3
    chans = TM.case_channels(P, -700 if P == 2400 else -1195, 4.0)
    iq = sources("lcg", bl, nb)
    t = make(R, T, P, bl, 2, chans)
    whole, y_whole = run_dev(t, iq)
    check_rules(whole, y_whole, iq, chans, TM.case_taps(T, P), P, "bit equality T %d P %d block_len %d" % (T, P, bl))
    t.reset()
    parts = [run_dev(t, iq[:, k:k + 1]) for k in range(nb)]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), whole)
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1).view(np.uint32), y_whole.view(np.uint32))
    t.reset()
    st = torch.cuda.Stream()
    other, y_other = run_dev(t, iq, stream=st)
    assert np.array_equal(other, whole) and np.array_equal(y_other.view(np.uint32), y_whole.view(np.uint32))
    t.reset()
    host = np.concatenate([t.run_host(iq[:, :2], 2), t.run_host(iq[:, 2:], 1)], axis=1)           # (the staging shrinks: kept)
    assert np.array_equal(host, whole)
    t.close()
    for c, ch in enumerate(chans):
        one = make(R, T, P, bl, 2, [ch])
        assert np.array_equal(run_dev(one, iq, want_y=False)[0][0], whole[c]), c
        one.close()
    # ... and a source's bytes alone: source 1 of 2 = the only source of a 1-source tuner
    solo = make(R, T, P, bl, 1, [(0, chans[1][1], chans[1][2])])
    assert np.array_equal(run_dev(solo, iq[1:2], want_y=False)[0][0], whole[1])
    solo.close()


def test_a_captured_graph_replays_to_the_bytes_of_the_plain_launch(R):
    """One torch stream, no branches: {tuner kernel, state kernel} of a 1-block launch captured once and replayed twice with the input refilled in
    between.  The state advances in place, so the second replay continues the first: bit-equal to two plain launches on a fresh object.  Inside a
    capture a channel cannot be set (FMD_E_STATE), and a launch whose stream differs from the previous launch's is refused; both leave the capture valid."""
    import torch
    T, P, bl, nb, reps = 64, 2400, RAGGED, 1, 2
    chans = TM.case_channels(P, -700, 1.0)
    iq = sources("lcg", bl, reps * nb)
    dev = torch.device("cuda:0")
    plain, graphed = make(R, T, P, bl, 2, chans), make(R, T, P, bl, 2, chans)
    want = [run_dev(plain, iq[:, r * nb:(r + 1) * nb]) for r in range(reps)]
    d_iq = torch.zeros((2, nb, bl), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((len(chans), nb, bl), dtype=torch.uint8, device=dev)
    d_y = torch.zeros((len(chans), nb, bl // 2, 2), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    ch = R.FmdTunerChannel(0, 5, 1.0, 0)
    with torch.cuda.graph(g, stream=st):
        graphed.run_device(d_iq, nb, d_out, d_y, hip_stream=st.cuda_stream)
        rc_set = R.lib().fmd_tuner_set_channel(graphed._h, 0, C.byref(ch))
        msg_set = R.lib().fmd_last_error().decode()
    assert rc_set == FMD_E_STATE and "captured" in msg_set, (rc_set, msg_set)
    for r in range(reps):
        d_iq.copy_(torch.from_numpy(np.ascontiguousarray(iq[:, r * nb:(r + 1) * nb])).to(dev))
        d_out.fill_(9)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want[r][0]), r
        assert np.array_equal(d_y.cpu().numpy().view(np.complex64)[..., 0].view(np.uint32), want[r][1].view(np.uint32)), r
    assert [bytes(graphed.get_state(s)) for s in range(2)] == [bytes(plain.get_state(s)) for s in range(2)]
    assert graphed.get_channel(0).shift == chans[0][1]                    # the refused set changed nothing
    # the previous launch on another stream: no event hand-over inside a capture
    graphed.run_device(d_iq, nb, d_out)                                   # the object's own stream
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        rc = R.lib().fmd_tuner_run_device(graphed._h, C.c_void_p(d_iq.data_ptr()), nb, C.c_void_p(d_out.data_ptr()), None, C.c_void_p(st.cuda_stream))
        msg = R.lib().fmd_last_error().decode()
        d_out.fill_(3)
    assert rc == FMD_E_STATE and "fmd_tuner_sync" in msg, (rc, msg)
    graphed.sync()
    g2.replay()
    torch.cuda.synchronize()
    assert bool((d_out == 3).all())
    plain.close()
    graphed.close()


# ---- 4. channels and state between launches ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,P,bl", [(64, 2400, 512), (16, 2400, 64), (64, 2400, RAGGED)])
def test_retune_between_launches(R, T, P, bl):
    """Shift, gain and source of every channel changed between two launches: the second launch is the model run with its own parameters over the
    carried raw history of the NEW source - no transient but the filter's own, because the state is the source's bytes and the mix is recomputed
    from the absolute index"""
    L = bl // 2
    first = [(0, -700, 1.0), (1, 100, 2.0), (1, 0, 1.0)]
    second = [(1, 250, 4.0), (0, -699, 1.0), (0, -1500, 0.5)]
    iq = sources("lcg", bl, 2)
    taps = TM.case_taps(T, P)
    t = make(R, T, P, bl, 2, first)
    out1, y1 = run_dev(t, iq[:, :1])
    check_rules(out1, y1, iq[:, :1], first, taps, P, "before the retune")
    for c, (src, sh, g) in enumerate(second):
        t.set_channel(c, src, sh, g)
        ch = t.get_channel(c)
        assert (ch.source, ch.shift, ch.gain) == (src, sh, g)
    out2, y2 = run_dev(t, iq[:, 1:])
    t.close()
    states = [(L % P, iq[s, 0, bl - 2 * T:].reshape(T, 2)) for s in range(2)]
    check_rules(out2, y2, iq[:, 1:], second, taps, P, "after the retune", states=states)
    # ... and equal to an object that ran the second set from the start
    u = make(R, T, P, bl, 2, second)
    both, _ = run_dev(u, iq)
    u.close()
    assert np.array_equal(both[:, 1:], out2)


@pytest.mark.parametrize("T,P,bl", [(64, 2400, 512), (16, 4, 64), (64, 4096, RAGGED)])
def test_state_hand_over_and_reset(R, T, P, bl):
    """get_state after 2 blocks is the model's (count, valid, the last T byte pairs); set_state into a fresh object, crossed over, continues bit-equal;
    reset zeroes it and what follows is a first launch again"""
    nb, k = 3, 2
    L = bl // 2
    shift = {2400: -700, 4: 3, 4096: -1195}[P]
    chans = [(0, shift, 1.0), (1, shift, 2.0)]
    iq = sources("lcg", bl, nb)
    t = make(R, T, P, bl, 2, chans)
    whole, _ = run_dev(t, iq)
    t.reset()
    first, _ = run_dev(t, iq[:, :k])
    states = [t.get_state(s) for s in range(2)]
    for s in range(2):
        assert (states[s].count, states[s].valid) == ((k * L) % P, 1)
        assert np.array_equal(np.array(states[s].hist[:2 * T], dtype=np.uint8), iq[s, k - 1, bl - 2 * T:])
    fresh = make(R, T, P, bl, 2, [(1, shift, 1.0), (0, shift, 2.0)])       # source s of fresh continues source 1 - s
    for s in range(2):
        fresh.set_state(s, states[1 - s])
    rest, _ = run_dev(fresh, iq[::-1, k:])
    assert np.array_equal(np.concatenate([first, rest], axis=1), whole)
    bad = R.FmdTunerState()
    bad.count = P
    assert R.lib().fmd_tuner_set_state(fresh._h, 0, C.byref(bad)) == FMD_E_ARG
    bad.count, bad.valid = 0, 2
    assert R.lib().fmd_tuner_set_state(fresh._h, 0, C.byref(bad)) == FMD_E_ARG
    fresh.reset()
    for s in range(2):
        assert not any(bytes(fresh.get_state(s)))
    again, _ = run_dev(fresh, iq[::-1])
    assert np.array_equal(again, whole)
    fresh.close()
    t.close()


def test_argument_checks_on_the_device(R):
    import torch
    T, P, bl = 64, 2400, 512
    t = make(R, T, P, bl, 2, [(0, 0, 1.0), (1, 0, 1.0)])
    L = R.lib()
    dev = torch.device("cuda:0")
    buf = torch.zeros(8 * bl + 64, dtype=torch.uint8, device=dev)
    d_y = torch.zeros(2 * bl + 16, dtype=torch.float32, device=dev)
    p = lambda off=0: C.c_void_p(buf.data_ptr() + off)  # noqa: E731
    assert buf.data_ptr() % 16 == 0
    assert L.fmd_tuner_run_device(t._h, p(4), 1, p(4 * bl), None, None) == FMD_E_ARG and b"16-byte" in L.fmd_last_error()
    assert L.fmd_tuner_run_device(t._h, p(), 1, p(4 * bl + 8), None, None) == FMD_E_ARG
    assert L.fmd_tuner_run_device(t._h, p(), 1, p(4 * bl), C.c_void_p(d_y.data_ptr() + 4), None) == FMD_E_ARG
    assert L.fmd_tuner_run_device(t._h, p(), -1, p(4 * bl), None, None) == FMD_E_ARG
    assert L.fmd_tuner_run_device(t._h, p(), 0, p(), None, None) == 0
    assert L.fmd_tuner_run_device(t._h, p(), 1, p(bl), None, None) == FMD_E_ARG and b"overlaps" in L.fmd_last_error()      # out inside in's 2 blocks
    assert L.fmd_tuner_run_device(t._h, p(2 * bl), 1, p(bl), None, None) == FMD_E_ARG                                      # in inside out's 2 blocks
    assert L.fmd_tuner_run_device(t._h, p(), 1, p(2 * bl), None, None) == 0                                                # adjacent: fine
    assert L.fmd_tuner_run_device(t._h, p(), 1 << 23, p(4 * bl), None, None) == FMD_E_ARG and b"too large" in L.fmd_last_error()
    t.sync()
    for src, sh, g in ((2, 0, 1.0), (-1, 0, 1.0), (0, 2400, 1.0), (0, -2400, 1.0), (0, 0, 0.0), (0, 0, 65.0), (0, 0, float("nan")), (0, 0, float("inf"))):
        ch = R.FmdTunerChannel(src, sh, g, 0)
        assert L.fmd_tuner_set_channel(t._h, 0, C.byref(ch)) == FMD_E_ARG and L.fmd_last_error(), (src, sh, g)
    ch = R.FmdTunerChannel(0, 0, 1.0, 0)
    assert L.fmd_tuner_set_channel(t._h, 2, C.byref(ch)) == FMD_E_ARG and L.fmd_tuner_get_channel(t._h, -1, C.byref(ch)) == FMD_E_ARG
    got = t.get_channel(1)
    assert (got.source, got.shift, got.gain) == (1, 0, 1.0)
    st = R.FmdTunerState()
    assert L.fmd_tuner_get_state(t._h, 2, C.byref(st)) == FMD_E_ARG and L.fmd_tuner_get_state(t._h, 1, C.byref(st)) == 0
    t.close()
