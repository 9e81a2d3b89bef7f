"""The capture spectrum on the device (fmd_batch_spectrum_device / _host; include/fmdemod_mi355x.h, "Capture spectrum"; csrc/spectrum.inc).

Held against the float64 model of tests/spectrum_model.py with the error of the float32 model as the yardstick (the rule of DESIGN.md section 2b:
rms within 2 x, worst value within 3 x of what a float32 reference loses against the same float64 model) and, bin by bin, against the bound
that the documented arithmetic allows (spectrum_model.spectrum_bound: the first rule's size is set by the block's strongest bin, the second
holds every weak bin to its own scale); bit-exact where the definition says the result depends on the block's bytes alone; and the
demodulator must not notice the calls.  The slot-edge shapes, the anchors and the launch shapes: tests/test_gpu_spectrum_edges.py.

Every stream gets an input of its own so that a stream mix-up shows: the oracle's DDS multiplex, the survey's LCG bytes, the quiet input of
test_gpu_levels.py (bytes in {127, 128}) and an off-bin tone of amplitude 0.9 at 0.1837 fs, which leaks into every bin."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spectrum_model import WINDOW_HANN, WINDOW_RECT, assert_bound_rule, spectrum_bound, spectrum_f32, spectrum_f64, tone_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

KW = dict(rate_in=300000, rate_out2=48000, mode=2)
KINDS = ("dds", "lcg", "quiet", "tone")
WORST = {"rms": 0.0, "max": 0.0}       # the largest share of either limit the kernel has used so far in this session (printed by every model test)


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@functools.lru_cache(maxsize=None)
def iq_of(kind, n_bytes):
    from oracle import dds_bytes, lcg_bytes
    if kind == "dds":
        a = dds_bytes(n_bytes, amp=100)
    elif kind == "lcg":
        a = lcg_bytes(n_bytes, 12345)[0]
    elif kind == "quiet":
        a = np.random.default_rng(7).integers(127, 129, n_bytes, dtype=np.uint8)
    elif kind == "tone":
        a = tone_bytes(n_bytes, 0.1837, amp=0.9)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def capture(kinds, nb, block_len):
    """u8 [len(kinds), nb, block_len], read-only"""
    a = np.stack([iq_of(k, nb * block_len).reshape(nb, block_len) for k in kinds])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def models(kinds, nb, block_len, n_bins, window):
    """(P64 float64 [S, nb, N], P32 float32 [S, nb, N]) of capture(kinds, nb, block_len), computed once"""
    iq = capture(kinds, nb, block_len)
    p64 = np.array([[spectrum_f64(iq[s, k], n_bins, window) for k in range(nb)] for s in range(len(kinds))])
    p32 = np.array([[spectrum_f32(iq[s, k], n_bins, window) for k in range(nb)] for s in range(len(kinds))])
    return p64, p32


@functools.lru_cache(maxsize=None)
def bounds(kinds, nb, block_len, n_bins, window):
    """the per-bin bound float64 [S, nb, N] of capture(kinds, nb, block_len), computed once"""
    iq = capture(kinds, nb, block_len)
    return np.array([[spectrum_bound(iq[s, k], n_bins, window)[1] for k in range(nb)] for s in range(len(kinds))])


def spectrum_dev(b, iq_np, n_bins, window=WINDOW_HANN, stream=None):
    """one fmd_batch_spectrum_device call over iq_np [S, nb, block_len] -> float32 [S, nb, n_bins] (numpy); stream: a torch stream or None"""
    import torch
    dev = torch.device("cuda:0")
    S, nb = iq_np.shape[0], iq_np.shape[1]
    iq = torch.from_numpy(np.array(iq_np, dtype=np.uint8).reshape(-1)).to(dev)
    out = torch.full((S, nb, n_bins), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.spectrum_device(iq, nb, n_bins, out, window=window, hip_stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    b.sync()
    return out.cpu().numpy()


def assert_model_rule(got, p64, p32, what):
    """rms(e_dev) <= 2 rms(e_ref) and max |e_dev| <= 3 max |e_ref| per (stream, block) over the N bins; prints the shares of the limits"""
    assert got.shape == p64.shape and got.dtype == np.float32
    assert np.isfinite(got).all() and (got >= 0).all(), what
    bad = []
    for s in range(got.shape[0]):
        for k in range(got.shape[1]):
            e_dev = got[s, k].astype(np.float64) - p64[s, k]
            e_ref = p32[s, k].astype(np.float64) - p64[s, k]
            rms_d, rms_r = np.sqrt((e_dev ** 2).mean()), np.sqrt((e_ref ** 2).mean())
            max_d, max_r = np.abs(e_dev).max(), np.abs(e_ref).max()
            assert rms_r > 0 and max_r > 0
            sh_rms, sh_max = rms_d / (2 * rms_r), max_d / (3 * max_r)
            WORST["rms"], WORST["max"] = max(WORST["rms"], sh_rms), max(WORST["max"], sh_max)
            print("%s stream %d block %d: rms %.3e (float32 model %.3e, %.0f %% of the limit), max %.3e (%.3e, %.0f %%)" %
                  (what, s, k, rms_d, rms_r, 100 * sh_rms, max_d, max_r, 100 * sh_max))
            if sh_rms > 1 or sh_max > 1:
                bad.append((s, k, sh_rms, sh_max))
    print("largest share of a limit so far: rms %.0f %%, max %.0f %%" % (100 * WORST["rms"], 100 * WORST["max"]))
    assert not bad, "%s: (stream, block, share of the rms limit, share of the max limit) beyond 1: %s" % (what, bad)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. against the float64 model --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [WINDOW_RECT, WINDOW_HANN])
@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_spectrum_matches_the_model(R, n_bins, window):
    """4 streams x 3 blocks of 10240 bytes: 20, 5 and 1 segments (five is no multiple of a worker count; one leaves a tail of 1024 samples).

    The tone (stream 3) is the case that decides the kernel's arithmetic: one bin carries the block's power, the
    float32 model happens to be right there to a fraction of a float32 step, and a float32 transform, one to three steps off, used 157 % of
    the rms limit and 105 % of the max limit (N = 256, rectangular, block 1).  The kernel computes in float64 and rounds once."""
    nb, bl = 3, 10240
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), len(KINDS))
    got = spectrum_dev(b, capture(KINDS, nb, bl), n_bins, window)
    b.close()
    assert_model_rule(got, *models(KINDS, nb, bl, n_bins, window), what="N %d window %d" % (n_bins, window))
    assert_bound_rule(got, models(KINDS, nb, bl, n_bins, window)[0], bounds(KINDS, nb, bl, n_bins, window), n_bins, window, "N %d window %d" % (n_bins, window))


@pytest.mark.parametrize("n_bins", [1024, 4096])
def test_spectrum_matches_the_model_on_full_blocks(R, n_bins):
    """2 streams x 2 blocks of 262144 bytes (128 and 32 segments), Hann"""
    nb, bl, kinds = 2, 262144, ("dds", "tone")
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), len(kinds))
    got = spectrum_dev(b, capture(kinds, nb, bl), n_bins, WINDOW_HANN)
    b.close()
    assert_model_rule(got, *models(kinds, nb, bl, n_bins, WINDOW_HANN), what="block_len 262144 N %d" % n_bins)
    assert_bound_rule(got, models(kinds, nb, bl, n_bins, WINDOW_HANN)[0], bounds(kinds, nb, bl, n_bins, WINDOW_HANN), n_bins, WINDOW_HANN,
                      "block_len 262144 N %d" % n_bins)


# ---- 2. bit-exact invariants -------------------------------------------------------------------------------------------------------------

def test_bit_exact_invariants(R):
    import torch
    nb, bl, N = 4, 10240, 1024
    iq = capture(KINDS, nb, bl)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), len(KINDS))
    first = spectrum_dev(b, iq, N)
    assert (first >= 0).all() and first.max() > 0
    assert same_bits(spectrum_dev(b, iq, N), first), "the same call twice"
    singles = np.concatenate([spectrum_dev(b, np.ascontiguousarray(iq[:, k:k + 1]), N) for k in range(nb)], axis=1)
    assert same_bits(singles, first), "one call of 4 blocks against 4 calls of 1 block"
    assert same_bits(b.spectrum_host(iq, nb, N), first), "spectrum_host against spectrum_device"
    assert same_bits(spectrum_dev(b, iq, N, stream=torch.cuda.Stream()), first), "an explicit stream against the batch's own"
    b.close()
    # a stream's bytes alone, and as stream 3 of 5 among other bytes
    b1 = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 1)
    alone = spectrum_dev(b1, iq[3:4], N)
    b1.close()
    assert same_bits(alone[0], first[3])
    five = np.stack([iq[1], iq[0], iq[2], iq[3], iq[1][::-1]])
    b5 = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 5)
    got5 = spectrum_dev(b5, five, N)
    b5.close()
    assert same_bits(got5[3], alone[0]), "alone against stream 3 of 5"
    assert same_bits(got5[0], first[1]) and same_bits(got5[1], first[0])


# ---- 3. ragged block ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins", [1024, 4096])
def test_ragged_block(R, n_bins):
    """block_len 200000 = 100000 samples: N = 1024 uses 97 segments and leaves 672 samples, N = 4096 uses 24 segments and leaves 1696"""
    bl = 200000
    iq = capture(KINDS, 1, bl)
    used = (bl // 2 // n_bins) * n_bins * 2          # bytes
    assert {1024: (97, 672), 4096: (24, 1696)}[n_bins] == (used // (2 * n_bins), (bl - used) // 2)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), len(KINDS))
    got = spectrum_dev(b, iq, n_bins)
    assert_model_rule(got, *models(KINDS, 1, bl, n_bins, WINDOW_HANN), what="block_len 200000 N %d" % n_bins)
    assert_bound_rule(got, models(KINDS, 1, bl, n_bins, WINDOW_HANN)[0], bounds(KINDS, 1, bl, n_bins, WINDOW_HANN), n_bins, WINDOW_HANN,
                      "block_len 200000 N %d" % n_bins)
    tail = iq.copy()
    tail[:, :, used:] ^= 0xFF
    assert same_bits(spectrum_dev(b, tail, n_bins), got), "the unused tail reached the spectrum"
    last = iq.copy()
    last[:, :, used - 1] ^= 0x40
    changed = spectrum_dev(b, last, n_bins)
    b.close()
    for s in range(len(KINDS)):
        assert not same_bits(changed[s], got[s]), "the last used byte of stream %d did not reach the spectrum" % s


# ---- 4. the demodulator does not notice --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", ["exact", "mfma_f"])
def test_the_demodulator_does_not_notice(R, math):
    import torch
    m = {"exact": R.MATH_EXACT, "mfma_f": R.MATH_FAST_MFMA_F}[math]
    bl, S, per, launches, N = 8192, 2, 2, 3, 1024
    cfg = R.wbfm_config(block_len=bl, math=m, **KW)
    iq_np = capture(("dds", "lcg"), per * launches, bl)
    dev = torch.device("cuda:0")
    parts = [torch.from_numpy(np.ascontiguousarray(iq_np[:, c * per:(c + 1) * per]).reshape(-1)).to(dev) for c in range(launches)]

    def run(with_spectrum):
        b = R.BatchDemod(cfg, S)
        assert b.math == m
        pcm = [torch.zeros(S * per * b.pcm_stride, dtype=torch.int16, device=dev) for _ in range(launches)]
        lens = [torch.zeros(S * per, dtype=torch.int32, device=dev) for _ in range(launches)]
        spec = [torch.full((S, per, N), -1.0, dtype=torch.float32, device=dev) for _ in range(launches + 1)]
        torch.cuda.synchronize()
        for c in range(launches):
            if with_spectrum:
                b.spectrum_device(parts[c], per, N, spec[c])
            b.run_device(parts[c], per, pcm[c], lens[c])
        if with_spectrum:
            b.spectrum_device(parts[0], per, N, spec[launches])
        b.sync()
        state = [bytes(b.get_state(s)) for s in range(S)]
        b.close()
        return [p.cpu().numpy() for p in pcm], [x.cpu().numpy() for x in lens], state, [x.cpu().numpy() for x in spec]

    p0, l0, s0, _ = run(False)
    p1, l1, s1, spec = run(True)
    assert all(np.array_equal(a, b) for a, b in zip(l0, l1)) and all(np.array_equal(a, b) for a, b in zip(p0, p1))
    assert s0 == s1
    assert any(x.any() for x in p0)
    fresh = R.BatchDemod(cfg, S)
    for c in range(launches):
        assert same_bits(spectrum_dev(fresh, iq_np[:, c * per:(c + 1) * per], N), spec[c]), c
    assert same_bits(spec[launches], spec[0])
    fresh.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_batch_working(R):
    import torch
    from oracle import OracleStream
    L = R.lib()
    dev = torch.device("cuda:0")

    def refused(b, bl, n_bins, window, offset, code):
        iq = torch.zeros(bl + 16, dtype=torch.uint8, device=dev)
        out = torch.zeros(max(n_bins, 1), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        rc = L.fmd_batch_spectrum_device(b._h, C.c_void_p(iq.data_ptr() + offset), 1, n_bins, window, C.c_void_p(out.data_ptr()), None)
        assert rc == code, (n_bins, window, offset, rc, L.fmd_last_error())
        return L.fmd_last_error().decode()

    for bl, cases in ((10240, [(96, 1, 0, -2), (8192, 1, 0, -2), (1024, 7, 0, -1), (1024, 1, 8, -1)]), (4096, [(4096, 1, 0, -1)])):
        b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 1)
        o = OracleStream(**KW)
        iq = iq_of("lcg", 4 * bl).reshape(4, bl)
        for k, (n_bins, window, offset, code) in enumerate(cases):
            msg = refused(b, bl, n_bins, window, offset, code)
            if code == -2:
                assert "256" in msg and "1024" in msg and "4096" in msg, msg       # the message names what is built
            want = o.block(iq[k])
            pcm, lens = b.run_host(iq[k].reshape(1, 1, bl), 1)
            assert lens[0, 0] == want.size and np.array_equal(pcm[0, 0, :want.size], want), (bl, k)
        with pytest.raises(R.FmdError):
            b.spectrum_host(iq[:1].reshape(1, 1, bl), 1, 96)
        b.close()
