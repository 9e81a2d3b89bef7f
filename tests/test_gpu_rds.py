"""The RDS receiver on the device (fmd_rds_*; include/fmdemod_mi355x.h, "RDS receiver"; csrc/rds.inc).

y and Tm are held to rds_model.y_bound / tm_bound against the float64 model of the same z and taps, the soft bits to soft_bound against the float64
slice given the device's own phi_b, counts and first-bit indices to equality (integers), phi to the float32 model's own error against float64
(DESIGN.md section 2b's rule: rms within 2x, worst within 3x, no additive term) on the synthesised RDS input, where |Ts| is well away from zero
(more than a quarter of the stream's largest) - and everything to bit equality wherever the header says the result depends on the
stream's z alone.  The bounds limit structure (tests/test_rds_cpu.py plants the defects they catch), they are no precision contest.

Shapes (rate_z, Tg, Bz): (18750, 64, 64) - the history is the whole block before, a block holds 4 bits, Pw = 300 does not divide Bz; (12000, 16,
112); (15000, 48, 256); (18750, 64, 1024) - one whole chunk; (18750, 64, 1280) - a block of two chunks, the second ragged."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rds_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(18750, 64, 64), (12000, 16, 112), (15000, 48, 256), (18750, 64, 1024), (18750, 64, 1280)]
AVG = 8
NZ = 3840                      # samples of z per stream in the model tests: 60, 34, 15, 3 and 3 blocks
WORST = {"y": 0.0, "tm": 0.0, "soft": 0.0}      # the largest shares of the bounds the kernels have used so far in this session


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@functools.lru_cache(maxsize=None)
def taps_of(rate_z, Tg):
    t = RM.design(rate_z, Tg).astype(np.float32)
    t.setflags(write=False)
    return t


groups_of = RM.groups_of
synth_z = RM.synth_z          # (rate_z, S, n): the synthesised RDS input, shared with tests/test_rds_cpu.py


@functools.lru_cache(maxsize=None)
def input_of(kind, rate_z, S, n):
    """complex64 [S, n], read-only; every stream its own values so that a stream mix-up shows"""
    if kind == "lcg":
        a = np.stack([RM.lcg_complex(n, 7 + 13 * s) for s in range(S)])
    elif kind == "zeros":
        a = np.zeros((S, n), dtype=np.complex64)
    elif kind == "rds":
        return synth_z(rate_z, S, n)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


def make(R, shape, S, max_blocks=64, taps=None):
    rate_z, Tg, Bz = shape
    return R.Rds(R.FmdRdsConfig(rate_z, Bz, Tg, AVG, max_blocks), S, taps=taps_of(rate_z, Tg) if taps is None else taps)


def run_dev(rds, z, stream=None):
    """one fmd_rds_run_device call over z complex64 [S, nb, Bz] -> dict of numpy arrays soft [S, nb, slot], lens, first, est [S, nb, 4]"""
    import torch
    dev = torch.device("cuda:0")
    S, nb = z.shape[0], z.shape[1]
    d_z = torch.from_numpy(np.ascontiguousarray(z).view(np.float32).reshape(-1).copy()).to(dev)
    d_soft = torch.full((S, nb, rds.bits_per_block), -7.0, dtype=torch.float32, device=dev)
    d_lens = torch.full((S, nb), -7, dtype=torch.int32, device=dev)
    d_first = torch.full((S, nb), -7, dtype=torch.int64, device=dev)
    d_est = torch.full((S, nb, 4), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rds.run_device(d_z, nb, d_soft, d_lens, d_first, d_est, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    rds.sync()
    return dict(soft=d_soft.cpu().numpy(), lens=d_lens.cpu().numpy(), first=d_first.cpu().numpy(), est=d_est.cpu().numpy())


def cat(parts):
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}


def same_bits(a, b):
    """two run_dev results (or arrays), bit for bit"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def state32_of(state):
    """the float32 model's form of a State"""
    o = state.copy()
    o.ts, o.zhist, o.yhist = np.complex64(o.ts), o.zhist.astype(np.complex64), o.yhist.astype(np.complex64)
    return o


def hold_to_the_model(got, y_dev, tm_dev, z, shape, what, state=None):
    """one stream from reset (or from the rds_model.State `state`): got = run_dev's arrays of that stream [nb, ..], y_dev complex64 [nb, Bz], tm_dev
    complex64 [nb], z complex64 [nb, Bz].  Returns (phi error of the device, of the float32 model, |Ts| of the float64 model) per block."""
    rate_z, Tg, Bz = shape
    geo, taps = RM.Geometry(rate_z, Bz), taps_of(rate_z, Tg)
    nb = z.shape[0]
    zf = z.reshape(-1)
    phi_dev = got["est"][:, 2].astype(np.float64)
    assert np.isfinite(got["soft"]).all() and np.isfinite(got["est"]).all() and (np.abs(phi_dev) <= 0.5).all() and (phi_dev < 0.5).all(), what
    start = RM.State(geo, Tg) if state is None else state
    m, _ = RM.receive(zf, geo, taps, AVG, state=start, phi_given=phi_dev)
    # integers: equal
    assert np.array_equal(got["lens"], m["counts"]) and np.array_equal(got["first"], m["first"]), (what, got["lens"], m["counts"])
    assert got["lens"].sum() == -(-(RM.Q * nb * Bz - start.e) // geo.two_rz) and got["lens"].max() <= geo.slot      # (from reset e = 2375 L)
    # y, Tm, the block's power
    br, bi = RM.y_bound(zf, taps, start.zhist)
    ey = y_dev.reshape(-1).astype(np.complex128) - m["y"]
    sy = max((np.abs(ey.real) / br).max(), (np.abs(ey.imag) / bi).max())
    bt = RM.tm_bound(m["y"], br, bi, Bz)
    et = tm_dev.astype(np.complex128) - m["tm"]
    st = max((np.abs(et.real) / bt).max(), (np.abs(et.imag) / bt).max())
    assert (np.abs(got["est"][:, 3] - m["pw"]) <= bt).all(), what
    # Ts: the one-pole over the device's own Tm, one fma per block
    ts = complex(start.ts)
    for b in range(nb):
        ts = (1 - 1 / AVG) * ts + complex(tm_dev[b])
        assert abs(got["est"][b, 0] - ts.real) <= 4 * RM.U * (abs(ts.real) + abs(tm_dev[b].real)) + 2.0 ** -126, (what, b)
        assert abs(got["est"][b, 1] - ts.imag) <= 4 * RM.U * (abs(ts.imag) + abs(tm_dev[b].imag)) + 2.0 ** -126, (what, b)
        ts = complex(got["est"][b, 0], got["est"][b, 1])
    # soft bits against the float64 slice with the device's phi
    yext = np.concatenate([start.yhist, m["y"]])
    byext = np.concatenate([np.zeros(geo.hy), np.maximum(br, bi)])       # (a carried y history is taken as exact: the callers carry zeros)
    es, counts, _ = RM.block_counts(geo, start.e, nb)
    ss = 0.0
    for b in range(nb):
        n = counts[b]
        assert not got["soft"][b, n:].view(np.uint32).any(), (what, b)             # the rest of the slot: +0
        if n:
            bs = RM.soft_bound(geo, yext[b * Bz:b * Bz + geo.hy + Bz], byext[b * Bz:b * Bz + geo.hy + Bz], es[b], n, phi_dev[b])
            ss = max(ss, float((np.abs(got["soft"][b, :n].astype(np.float64) - m["soft"][b]) / bs).max()))
    for k, v in (("y", sy), ("tm", st), ("soft", ss)):
        WORST[k] = max(WORST[k], v)
    print("%s: share of the bounds y %.4f Tm %.4f soft %.4f (largest so far %.4f %.4f %.4f)" % (what, sy, st, ss, WORST["y"], WORST["tm"], WORST["soft"]))
    assert sy < 1 and st < 1 and ss < 1, (what, sy, st, ss)
    m32, _ = RM.receive(zf, geo, taps, AVG, dtype=np.float32, state=None if state is None else state32_of(state))
    wrap = lambda d: (d + 0.5) % 1.0 - 0.5  # noqa: E731
    return wrap(phi_dev - m["phi"]), wrap(m32["phi"].astype(np.float64) - m["phi"]), np.abs(m["ts"])


# ---- 1. against the float64 model --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_rds_receiver_matches_the_model(R, shape):
    rate_z, Tg, Bz = shape
    S, nb = 3, NZ // Bz
    rds = make(R, shape, S)
    geo = RM.Geometry(rate_z, Bz)
    assert rds.bits_per_block == geo.slot
    for kind in ("lcg", "zeros", "rds"):
        z = input_of(kind, rate_z, S, NZ)[:, :nb * Bz].reshape(S, nb, Bz)
        rds.reset()
        got = run_dev(rds, z)
        y_dev, tm_dev = rds.last_y(nb)
        e_dev, e_ref, mag = [], [], []
        for s in range(S):
            a, b, c = hold_to_the_model({k: v[s] for k, v in got.items()}, y_dev[s], tm_dev[s], z[s], shape, "%s %s stream %d" % (kind, shape, s))
            e_dev.append(a); e_ref.append(b); mag.append(c / max(c.max(), 1e-300))
        if kind == "zeros":
            assert not got["soft"].view(np.uint32).any() and not got["est"][..., :2].any() and not y_dev.view(np.uint32).any()
        if kind == "rds":
            e_dev, e_ref, mag = np.concatenate(e_dev), np.concatenate(e_ref), np.concatenate(mag)
            keep = mag > 0.25                                              # |Ts| well away from zero (a quarter of the stream's largest): past the fill
            rms = lambda x: float(np.sqrt(np.mean(x * x)))  # noqa: E731
            print("phi %s: %d blocks, device rms %.3g worst %.3g; float32 model rms %.3g worst %.3g" %
                  (shape, keep.sum(), rms(e_dev[keep]), np.abs(e_dev[keep]).max(), rms(e_ref[keep]), np.abs(e_ref[keep]).max()))
            assert keep.sum() >= 6
            assert rms(e_dev[keep]) <= 2 * rms(e_ref[keep])
            assert np.abs(e_dev[keep]).max() <= 3 * np.abs(e_ref[keep]).max()
    rds.close()


# ---- 2. bit equality: the result depends on the stream's z alone ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_split_invariance(R, shape):
    """6 blocks in one call = 1 + 2 + 3 across calls = six single calls; stream s of a 3-stream object = a 1-stream object fed the same z; the host
    form; and the state after is the same bytes"""
    rate_z, Tg, Bz = shape
    S, nb = 3, 6
    z = input_of("rds", rate_z, S, 6 * Bz).reshape(S, nb, Bz)
    rds = make(R, shape, S)
    whole = run_dev(rds, z)
    states = [bytes(rds.get_state(s)) for s in range(S)]
    assert whole["lens"].min() >= 0 and whole["soft"].any()
    rds.reset()
    assert same_bits(cat([run_dev(rds, z[:, 0:1]), run_dev(rds, z[:, 1:3]), run_dev(rds, z[:, 3:6])]), whole)
    assert [bytes(rds.get_state(s)) for s in range(S)] == states
    rds.reset()
    assert same_bits(cat([run_dev(rds, z[:, k:k + 1]) for k in range(nb)]), whole)
    assert [bytes(rds.get_state(s)) for s in range(S)] == states
    rds.reset()
    soft, lens, first, est = rds.run_host(z[:, :4], 4)
    soft2, lens2, first2, est2 = rds.run_host(z[:, 4:], 2)
    host = dict(soft=np.concatenate([soft, soft2], axis=1), lens=np.concatenate([lens, lens2], axis=1), first=np.concatenate([first, first2], axis=1),
                est=np.concatenate([est, est2], axis=1))
    assert same_bits(host, whole)
    rds.close()
    for s in range(S):
        one = make(R, shape, 1)
        assert same_bits(run_dev(one, z[s:s + 1]), {k: v[s:s + 1] for k, v in whole.items()}), s
        assert bytes(one.get_state(0)) == states[s]
        one.close()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_state_hand_over(R, shape):
    """get_state after k blocks is the model's integers and the last Tg z; set_state into a fresh object, streams crossed over, continues bit-equal;
    an out-of-range state is refused; reset zeroes it"""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    S, nb, k = 2, 5, 3
    z = input_of("rds", rate_z, S, 6 * Bz)[:, :nb * Bz].reshape(S, nb, Bz)
    rds = make(R, shape, S)
    whole = run_dev(rds, z)
    rds.reset()
    first = run_dev(rds, z[:, :k])
    states = [rds.get_state(s) for s in range(S)]
    for s in range(S):
        _, st = RM.receive(z[s, :k].reshape(-1), geo, taps_of(rate_z, Tg), AVG)
        assert (states[s].phase, states[s].frac + RM.Q * geo.lb, states[s].bit) == (st.phase, st.e, st.bit) and st.phase == (k * Bz) % geo.pw
        assert np.array_equal(np.array(states[s].zhist[:2 * Tg], dtype=np.float32).view(np.complex64), z[s, k - 1, Bz - Tg:])
        assert (states[s].ts[0], states[s].ts[1]) == (first["est"][s, k - 1, 0], first["est"][s, k - 1, 1])
    fresh = make(R, shape, S)
    for s in range(S):
        fresh.set_state(s, states[S - 1 - s])
    rest = run_dev(fresh, z[::-1, k:])
    assert same_bits(cat([first, {k_: v[::-1] for k_, v in rest.items()}]), whole)
    bad = R.FmdRdsState()
    bad.phase = geo.pw
    assert R.lib().fmd_rds_set_state(fresh._h, 0, C.byref(bad)) == -1
    bad.phase, bad.frac = 0, geo.two_rz - RM.Q * geo.lb
    assert R.lib().fmd_rds_set_state(fresh._h, 0, C.byref(bad)) == -1
    fresh.reset()
    assert not any(bytes(fresh.get_state(0))) and not any(bytes(fresh.get_state(1)))
    assert same_bits(run_dev(fresh, z), whole)
    fresh.close()
    rds.close()


def test_the_callers_stream_the_objects_stream_and_a_captured_graph(R):
    """Launches alternate between a caller's stream and the object's own (the library orders them with an event): bit-equal to one stream
    throughout.  Then the four kernels of a 2-block launch captured once and replayed three times with z refilled in between: the state advances
    in place, so replay r continues replay r - 1, bit-equal to eager launches.  A launch whose stream differs from the previous launch's is
    refused inside a capture (FMD_E_STATE) and leaves the capture valid."""
    import torch
    shape = SHAPES[0]
    rate_z, Tg, Bz = shape
    S, nb, reps = 3, 2, 3
    z = input_of("rds", rate_z, S, NZ)[:, :reps * nb * Bz].reshape(S, reps, nb, Bz)
    dev = torch.device("cuda:0")
    eager, mixed, graphed = make(R, shape, S), make(R, shape, S), make(R, shape, S)
    want = [run_dev(eager, z[:, r]) for r in range(reps)]
    st = torch.cuda.Stream()
    for r in range(reps):
        assert same_bits(run_dev(mixed, z[:, r], stream=st if r != 1 else None), want[r]), r
    assert [bytes(mixed.get_state(s)) for s in range(S)] == [bytes(eager.get_state(s)) for s in range(S)]
    d_z = torch.zeros((S, nb, Bz, 2), dtype=torch.float32, device=dev)
    d_soft = torch.zeros((S, nb, graphed.bits_per_block), dtype=torch.float32, device=dev)
    d_lens = torch.zeros((S, nb), dtype=torch.int32, device=dev)
    d_first = torch.zeros((S, nb), dtype=torch.int64, device=dev)
    d_est = torch.zeros((S, nb, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        graphed.run_device(d_z, nb, d_soft, d_lens, d_first, d_est, hip_stream=st.cuda_stream)
    for r in range(reps):
        d_z.copy_(torch.from_numpy(np.ascontiguousarray(z[:, r]).view(np.float32).reshape(S, nb, Bz, 2).copy()).to(dev))
        d_soft.fill_(-1.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = dict(soft=d_soft.cpu().numpy(), lens=d_lens.cpu().numpy(), first=d_first.cpu().numpy(), est=d_est.cpu().numpy())
        assert same_bits(got, want[r]), r
    assert [bytes(graphed.get_state(s)) for s in range(S)] == [bytes(eager.get_state(s)) for s in range(S)]
    graphed.run_device(d_z, nb, d_soft, d_lens, d_first, d_est)            # the object's own stream
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        rc = R.lib().fmd_rds_run_device(graphed._h, C.c_void_p(d_z.data_ptr()), nb, C.c_void_p(d_soft.data_ptr()), C.c_void_p(d_lens.data_ptr()), None, None,
                                        C.c_void_p(st.cuda_stream))
        msg = R.lib().fmd_last_error().decode()
        d_soft.fill_(3.0)
    assert rc == -6 and "fmd_rds_sync" in msg, (rc, msg)
    graphed.sync()
    g2.replay()
    torch.cuda.synchronize()
    assert bool((d_soft == 3.0).all())
    for o in (eager, mixed, graphed):
        o.close()


def test_argument_checks_on_the_device(R):
    import torch
    shape = SHAPES[2]
    rds = make(R, shape, 1, max_blocks=2)
    L = R.lib()
    dev = torch.device("cuda:0")
    d_z = torch.zeros(2 * 2 * 256 + 8, dtype=torch.float32, device=dev)
    d_soft = torch.zeros(2 * rds.bits_per_block + 8, dtype=torch.float32, device=dev)
    d_lens = torch.zeros(8, dtype=torch.int32, device=dev)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.fmd_rds_run_device(rds._h, p(d_z, 8), 1, p(d_soft), p(d_lens), None, None, None) == -1 and b"16-byte" in L.fmd_last_error()
    assert L.fmd_rds_run_device(rds._h, p(d_z), 1, p(d_soft, 4), p(d_lens), None, None, None) == -1
    assert L.fmd_rds_run_device(rds._h, p(d_z), -1, p(d_soft), p(d_lens), None, None, None) == -1
    assert L.fmd_rds_run_device(rds._h, p(d_z), 0, p(d_soft), p(d_lens), None, None, None) == 0
    assert L.fmd_rds_run_device(rds._h, p(d_z), 3, p(d_soft), p(d_lens), None, None, None) == -1 and b"max_blocks" in L.fmd_last_error()
    assert L.fmd_rds_run_device(rds._h, p(d_z), 2, p(d_soft), p(d_lens), None, None, None) == 0
    st = R.FmdRdsState()
    assert L.fmd_rds_get_state(rds._h, 1, C.byref(st)) == -1 and L.fmd_rds_get_state(rds._h, 0, C.byref(st)) == 0
    rds.close()
    h = C.c_void_p()
    cfg = R.FmdRdsConfig(18750, 32, 16, 8, 4)                               # a block shorter than the lookback
    assert L.fmd_rds_create(C.byref(h), C.byref(cfg), None, 1, -1) == -2


# ---- 3. end to end on the device -----------------------------------------------------------------------------------------------------------------------

def decode(R, soft, lens):
    """the decoder over one stream's slots in order"""
    dec = R.RdsDecoder()
    got = []
    for b in range(soft.shape[0]):
        got += dec.push(soft[b, :lens[b]])
    return dec, got


def test_end_to_end_from_a_synthesised_multiplex(R):
    """Two streams, two PIs and names: MPX v at 300 k (RDS at 0.04 and 0.05 beside a pilot and a tone), 24 blocks of M = 16384 -> fmd_subc (57 kHz,
    2.4 kHz, 128 taps, D 16) -> fmd_rds (64 taps, avg_blocks 8) in launches of 8 blocks on one stream -> decoder.  Every group but the first 3 comes
    out, in order, all four blocks ok, none wrong; PI and PS are read."""
    import torch
    rate, D, M, nb, S = 300000, 16, 16384, 24, 2
    ident = [(0x1234, "RADIO 42"), (0xD3A5, "HELLO FM")]
    sent = [groups_of(12, *ident[s]) for s in range(S)]
    v = np.stack([RM.mpx(RM.data_bits(sent[s]), rate, nb * M, level=0.04 + 0.01 * s, phase=0.7 + 2 * s, t0=3.0 + 0.4 * s) for s in range(S)]).astype(np.float32)
    dev = torch.device("cuda:0")
    sub = R.Subcarrier(R.FmdSubcConfig(rate, 57000, 2400, 128, D, M), S)
    rds = R.Rds.from_subcarrier(sub, n_taps=64, avg_blocks=8, max_blocks=8)
    assert (rds.cfg.rate_z, rds.cfg.block_z, rds.n_streams) == (18750, 1024, S)
    d_v = [torch.from_numpy(np.ascontiguousarray(v.reshape(S, nb, M)[:, a:a + 8])).to(dev) for a in range(0, nb, 8)]
    d_z = torch.zeros((S, 8, M // D, 2), dtype=torch.float32, device=dev)
    d_soft = torch.zeros((S, 8, rds.bits_per_block), dtype=torch.float32, device=dev)
    d_lens = torch.zeros((S, 8), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    soft, lens = [], []
    for a in range(0, nb, 8):
        sub.run_device(d_v[a // 8], 8, d_z, hip_stream=st.cuda_stream)
        rds.run_device(d_z, 8, d_soft, d_lens, hip_stream=st.cuda_stream)
        st.synchronize()
        soft.append(d_soft.cpu().numpy())
        lens.append(d_lens.cpu().numpy())
    soft, lens = np.concatenate(soft, axis=1), np.concatenate(lens, axis=1)
    for s in range(S):
        dec, got = decode(R, soft[s], lens[s])
        full = [g[:4] for g in got if g[4] == 15]
        print("stream %d: %d groups out, %d whole, the first whole one is sent group %d" % (s, len(got), len(full), sent[s].index(full[0])))
        assert all(g in sent[s] for g in full) and full == sent[s][12 - len(full):] and len(full) >= 9
        assert (dec.pi, dec.ps) == ident[s]
    rds.close()
    sub.close()


def test_end_to_end_from_fm_modulated_iq(R):
    """One stream of u8 IQ, ten blocks of 262144 bytes at 2.4 MS/s: a carrier at -fs/4 frequency-modulated with the multiplex (the deviation that makes
    the discriminator read the multiplex's own values; amplitude 100, dithered) -> the stereo batch's `v` tap -> Batch.subcarrier(57000, 2400) ->
    Rds.from_subcarrier -> decoder.  0.55 s holds six groups: the fourth and fifth come out whole, nothing wrong comes out, and the PI is read."""
    import torch
    fs, bl, nb = 2400000, 262144, 10
    n = nb * bl // 2
    sent = groups_of(7, 0xC0DE, "IQ TEST ")
    mpx = RM.mpx(RM.data_bits(sent), fs, n, level=0.05, t0=3.0)
    ph = np.cumsum(mpx / 8.0 - np.pi / 2)
    rng = np.random.default_rng(9)
    iq = np.empty(2 * n, dtype=np.uint8)
    iq[0::2] = np.clip(np.floor(128 + 100 * np.cos(ph) + rng.random(n)), 0, 255)
    iq[1::2] = np.clip(np.floor(128 + 100 * np.sin(ph) + rng.random(n)), 0, 255)
    dev = torch.device("cuda:0")
    b = R.BatchDemod(R.wbfm_config(rate_in=300000, rate_out2=48000, mode=2, block_len=bl, math=R.MATH_FAST), 1)
    d_iq = torch.from_numpy(iq).to(dev)
    pcm = torch.zeros(nb * b.pcm_stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(nb, dtype=torch.int32, device=dev)
    v = torch.zeros((1, nb, bl // 16), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.run_device(d_iq, nb, pcm, lens, debug={"v": v})
    b.sync()
    sub = b.subcarrier(57000, 2400)
    rds = R.Rds.from_subcarrier(sub, max_blocks=nb)
    z = torch.zeros((1, nb, sub.out_per_block, 2), dtype=torch.float32, device=dev)
    d_soft = torch.zeros((1, nb, rds.bits_per_block), dtype=torch.float32, device=dev)
    d_lens = torch.zeros((1, nb), dtype=torch.int32, device=dev)
    d_est = torch.zeros((1, nb, 4), dtype=torch.float32, device=dev)
    sub.run_device(v, nb, z)
    sub.sync()
    rds.run_device(z, nb, d_soft, d_lens, None, d_est)
    rds.sync()
    level = float(np.sqrt(d_est.cpu().numpy()[0, 2:, 3].mean() / 1024))
    dec, got = decode(R, d_soft.cpu().numpy()[0], d_lens.cpu().numpy()[0])
    full = [g[:4] for g in got if g[4] == 15]
    print("rms |y| %.4f; %d groups out, whole: %s" % (level, len(got), [sent.index(g) if g in sent else -1 for g in full]))
    assert all(g in sent for g in full) and sent[3] in full and sent[4] in full
    assert dec.pi == 0xC0DE
    for g in got:
        assert any(all(g[p] == s[p] for p in range(4) if g[4] & (1 << p)) for s in sent)
    for o in (rds, sub, b):
        o.close()
