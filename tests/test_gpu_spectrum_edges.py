"""The capture spectrum on the device at the shapes its decomposition makes special, against anchors that do not go through np.fft, and in the
launch shapes the header promises (include/fmdemod_mi355x.h, "Capture spectrum"; csrc/spectrum.inc).  Beside tests/test_gpu_spectrum.py.

A workgroup holds G = 4096 / N segment slots; slot g takes segments g, g + G, ... and prefetches its next one; the G partial spectra are added
through LDS at the end.  So: one segment with G - 1 idle slots, G - 1, G, G + 1 and 2 G + 1 segments, a block that fits exactly and the smallest
tail (spectrum_model.EDGE_BLOCK_LENS) - each with six inputs (one per (stream, block) of 3 streams x 2 blocks), both windows and every n_bins
that fits, on ONE batch per block_len (so a batch holds up to six (n_bins, window) tables).

Two rules in every model test: the rms / worst-value rule of tests/test_gpu_spectrum.py (the float32 model's error as the yardstick) and the
per-bin bound of spectrum_model.spectrum_bound.  Where the float32 model loses nothing (the square wave with the rectangular window and a
power-of-two segment count: its error is exactly zero) the first rule's limits are zero and the device must be exact as well."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spectrum_model import (EDGE_BLOCK_LENS, EDGE_KINDS, EPS_PATH, WEAK_FREQ, WINDOW_HANN, WINDOW_RECT, assert_bound_rule, input_bytes,  # noqa: E402
                            samples_f64, spectrum_bound, spectrum_f32, tone_bytes)

pytestmark = pytest.mark.gpu

KW = dict(rate_in=300000, rate_out2=48000, mode=2)
S, NB = 3, 2                           # slot (s, k) carries EDGE_KINDS[2 s + k]
ALL_LENS = sorted({bl for v in EDGE_BLOCK_LENS.values() for bl in v})
WORST = {"rms": 0.0, "max": 0.0}


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@functools.lru_cache(maxsize=None)
def iq_of(kind, n_bytes):
    a = input_bytes(kind, n_bytes)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def edge_capture(block_len):
    """u8 [3, 2, block_len], read-only: the first block_len bytes of each of the six kinds"""
    a = np.stack([iq_of(k, block_len) for k in EDGE_KINDS]).reshape(S, NB, block_len)
    a.setflags(write=False)
    return a


def models_of(iq, n_bins, window):
    """(P64, P32, bound), each [S, nb, N], of iq u8 [S, nb, block_len]"""
    pb = [[spectrum_bound(iq[s, k], n_bins, window) for k in range(iq.shape[1])] for s in range(iq.shape[0])]
    p32 = np.array([[spectrum_f32(iq[s, k], n_bins, window) for k in range(iq.shape[1])] for s in range(iq.shape[0])])
    return np.array([[x[0] for x in row] for row in pb]), p32, np.array([[x[1] for x in row] for row in pb])


@functools.lru_cache(maxsize=None)
def edge_models(block_len, n_bins, window):
    return models_of(edge_capture(block_len), n_bins, window)


def spectrum_dev(b, iq_np, n_bins, window=WINDOW_HANN):
    """one fmd_batch_spectrum_device call over iq_np [S, nb, block_len] on the batch's own stream -> float32 [S, nb, n_bins] (numpy)"""
    import torch
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(np.array(iq_np, dtype=np.uint8).reshape(-1)).to(dev)
    out = torch.full((iq_np.shape[0], iq_np.shape[1], n_bins), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.spectrum_device(iq, iq_np.shape[1], n_bins, out, window=window)
    b.sync()
    return out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_rules(got, p64, p32, bound, n_bins, window, what):
    """The rule of tests/test_gpu_spectrum.py - rms(e_dev) <= 2 rms(e_ref) and max |e_dev| <= 3 max |e_ref| per (stream, block) - and the per-bin
    bound.  e_ref == 0 (see the module's docstring) leaves the first rule's limits at zero: e_dev must be zero too."""
    assert got.shape == p64.shape and got.dtype == np.float32
    assert np.isfinite(got).all() and (got >= 0).all(), what
    bad = []
    for s in range(got.shape[0]):
        for k in range(got.shape[1]):
            e_dev = got[s, k].astype(np.float64) - p64[s, k]
            e_ref = p32[s, k].astype(np.float64) - p64[s, k]
            rms_d, rms_r = np.sqrt((e_dev ** 2).mean()), np.sqrt((e_ref ** 2).mean())
            max_d, max_r = np.abs(e_dev).max(), np.abs(e_ref).max()
            if max_r == 0:
                print("%s stream %d block %d: the float32 model is exact; device rms %.3e, max %.3e" % (what, s, k, rms_d, max_d))
                if max_d != 0:
                    bad.append((s, k, rms_d, max_d))
                continue
            sh_rms, sh_max = rms_d / (2 * rms_r), max_d / (3 * max_r)
            WORST["rms"], WORST["max"] = max(WORST["rms"], sh_rms), max(WORST["max"], sh_max)
            print("%s stream %d block %d: rms %.3e (float32 model %.3e, %.0f %% of the limit), max %.3e (%.3e, %.0f %%)" %
                  (what, s, k, rms_d, rms_r, 100 * sh_rms, max_d, max_r, 100 * sh_max))
            if sh_rms > 1 or sh_max > 1:
                bad.append((s, k, sh_rms, sh_max))
    print("largest share of a limit so far: rms %.0f %%, max %.0f %%" % (100 * WORST["rms"], 100 * WORST["max"]))
    assert not bad, "%s: (stream, block, share of the rms limit, share of the max limit; or the errors where the limits are zero): %s" % (what, bad)
    assert_bound_rule(got, p64, bound, n_bins, window, what)


# ---- B. slot-edge shapes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_len", ALL_LENS)
def test_slot_edge_shapes(R, block_len):
    """Six inputs x every n_bins that fits x both windows on one batch: both rules; Parseval with the rectangular window against the bytes
    (|sum_k P_dev[k] - mean |x|^2 of the used samples| <= sum_k bound[k]); the unused tail (where there is one) does not reach P, the last used
    byte reaches every (stream, block)."""
    iq = edge_capture(block_len)
    b = R.BatchDemod(R.wbfm_config(block_len=block_len, **KW), S)
    pairs = 0
    for n_bins in (256, 1024, 4096):
        if n_bins > block_len // 2:
            continue
        nseg = block_len // 2 // n_bins
        used = nseg * n_bins * 2                    # bytes
        for window in (WINDOW_RECT, WINDOW_HANN):
            what = "block_len %d N %d (%d segments, tail %d) window %d" % (block_len, n_bins, nseg, (block_len - used) // 2, window)
            p64, p32, bound = edge_models(block_len, n_bins, window)
            got = spectrum_dev(b, iq, n_bins, window)
            pairs += 1
            assert_rules(got, p64, p32, bound, n_bins, window, what)
            if window == WINDOW_RECT:
                for s in range(S):
                    for k in range(NB):
                        mean2 = (np.abs(samples_f64(iq[s, k, :used])) ** 2).mean()
                        assert abs(got[s, k].astype(np.float64).sum() - mean2) <= bound[s, k].sum(), (what, s, k)
            if used < block_len:
                tail = iq.copy()
                tail[:, :, used:] ^= 0xFF
                assert same_bits(spectrum_dev(b, tail, n_bins, window), got), what + ": the unused tail reached the spectrum"
            last = iq.copy()
            last[:, :, used - 1] ^= 0x40
            changed = spectrum_dev(b, last, n_bins, window)
            for s in range(S):
                for k in range(NB):
                    assert not same_bits(changed[s, k], got[s, k]), what + ": the last used byte of stream %d block %d did not reach the spectrum" % (s, k)
    assert pairs == (6 if block_len >= 8192 else 4 if block_len >= 2048 else 2)
    b.close()


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_equal_segments_in_every_slot(R, n_bins):
    """block_len = 2 N G with the same segment bytes G times: every slot adds the same double, G is a power of two and so is the ratio of the two
    scales, so P is bit-equal to the one-segment block's"""
    G = 4096 // n_bins
    one = np.stack([iq_of(k, 2 * n_bins) for k in EDGE_KINDS]).reshape(S, NB, 2 * n_bins)
    rep = np.ascontiguousarray(np.tile(one, (1, 1, G)))
    assert rep.shape == (S, NB, 8192) and np.array_equal(rep[:, :, -2 * n_bins:], one)
    b1 = R.BatchDemod(R.wbfm_config(block_len=2 * n_bins, **KW), S)
    bG = R.BatchDemod(R.wbfm_config(block_len=8192, **KW), S)
    for window in (WINDOW_RECT, WINDOW_HANN):
        a = spectrum_dev(b1, one, n_bins, window)
        assert a.max() > 0
        assert same_bits(spectrum_dev(bG, rep, n_bins, window), a), (n_bins, window)
    b1.close()
    bG.close()


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_a_constant_byte(R, n_bins):
    """x = c (1 + j), c = (u - 127.5) / 128: with w = 1 all of 2 c^2 on bin 0; with Hann 2/3 of it on bin 0 and 1/6 each on bins 1 and N - 1 (the
    window's own three lines over sum w^2 = 3 N / 8); every other bin is zero.  Each bin within its bound of that."""
    consts = (0, 255, 127, 128, 1, 200)
    bl = 16384
    iq = np.stack([np.full(bl, u, np.uint8) for u in consts]).reshape(S, NB, bl)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), S)
    for window in (WINDOW_RECT, WINDOW_HANN):
        got = spectrum_dev(b, iq, n_bins, window)
        for j, u in enumerate(consts):
            p = 2.0 * ((u - 127.5) / 128.0) ** 2
            want = np.zeros(n_bins)
            if window == WINDOW_RECT:
                want[0] = p
            else:
                want[0], want[1], want[n_bins - 1] = 2.0 * p / 3.0, p / 6.0, p / 6.0
            bound = spectrum_bound(iq[j // NB, j % NB], n_bins, window)[1]
            err = np.abs(got[j // NB, j % NB].astype(np.float64) - want)
            print("byte %d N %d window %d: P[0] %.9g (want %.9g), worst share of the bound %.3f" % (u, n_bins, window, got[j // NB, j % NB, 0], want[0], (err / bound).max()))
            assert (err <= bound).all(), (u, n_bins, window, int((err / bound).argmax()), float((err / bound).max()))
    b.close()


# ---- C. anchors that do not go through np.fft --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_bins,k0", [(256, 37), (1024, 700), (4096, 1)])
def test_a_bin_centred_tone_on_the_device(R, n_bins, k0):
    """Amplitude 0.9 at +k0 / N peaks at bin k0, at -k0 / N at bin N - k0 (both windows); with the rectangular window the peak equals a float64
    dot product of the bytes with e^(-2 pi i k0 n / N), written out here, within the bound of that bin (made from the same dot product)."""
    nseg = 3
    bl = nseg * 2 * n_bins
    iq = np.stack([tone_bytes(bl, k0 / n_bins, amp=0.9), tone_bytes(bl, -k0 / n_bins, amp=0.9)]).reshape(2, 1, bl)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 2)
    for window in (WINDOW_RECT, WINDOW_HANN):
        got = spectrum_dev(b, iq, n_bins, window)
        for s, peak in ((0, k0), (1, n_bins - k0)):
            assert int(got[s, 0].argmax()) == peak, (window, s)
            if window == WINDOW_RECT:
                x = samples_f64(iq[s, 0]).reshape(nseg, n_bins)
                e = np.exp(-2j * np.pi * ((peak * np.arange(n_bins)) % n_bins) / n_bins)
                X = (x * e).sum(axis=1)
                A = np.abs(x).sum(axis=1)
                scale = 1.0 / (nseg * n_bins * n_bins)
                want = (np.abs(X) ** 2).sum() * scale
                d = scale * (2.0 * np.abs(X) * EPS_PATH * A + (EPS_PATH * A) ** 2).sum()
                bound = d + 2.0 ** -24 * (want + d) + 2.0 ** -149
                err = abs(float(got[s, 0, peak]) - want)
                print("N %d bin %d: P %.9g, dot product %.9g, error %.3e, bound %.3e" % (n_bins, peak, got[s, 0, peak], want, err, bound))
                assert err <= bound and want == pytest.approx(0.81, rel=0.02)
    b.close()


@functools.lru_cache(maxsize=None)
def full_block_capture():
    a = np.stack([iq_of("dds", 262144), iq_of("strong_weak", 262144)]).reshape(2, 1, 262144)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("n_bins", [256, 1024, 4096])
def test_full_blocks_the_multiplex_peak_and_the_weak_tone(R, n_bins):
    """262144 bytes: the oracle's DDS multiplex peaks at bin 197 / 747 / 3149 (rectangular, the header's figures); the tone 50 dB below the strong
    one stands more than 100 x over the block's median bin (Hann, N = 1024 and 4096: 4.3e-6 to 4.6e-6 over 2e-8 and 5e-9); both rules."""
    iq = full_block_capture()
    b = R.BatchDemod(R.wbfm_config(block_len=262144, **KW), 2)
    for window in (WINDOW_RECT, WINDOW_HANN):
        got = spectrum_dev(b, iq, n_bins, window)
        assert_rules(got, *full_block_models(n_bins, window), n_bins, window, "block_len 262144 N %d window %d" % (n_bins, window))
        if window == WINDOW_RECT:
            assert int(got[0, 0].argmax()) == {256: 197, 1024: 747, 4096: 3149}[n_bins]
        elif n_bins >= 1024:
            k = int(round((1 + WEAK_FREQ) * n_bins))
            weak, median = float(got[1, 0, k - 2:k + 3].max()), float(np.median(got[1, 0]))
            print("N %d: the weak tone reads %.3e near bin %d over a median bin of %.3e" % (n_bins, weak, k, median))
            assert weak > 100 * median
    b.close()


@functools.lru_cache(maxsize=None)
def full_block_models(n_bins, window):
    return models_of(full_block_capture(), n_bins, window)


# ---- D. launch shapes --------------------------------------------------------------------------------------------------------------------

def test_a_grid_beyond_65535_workgroups(R):
    """8 streams x 8750 blocks of 512 bytes, N = 256: 70 000 workgroups, 36 MB in, 72 MB out.  Slot j carries block j mod 7 of seven LCG blocks;
    every slot's P is bit-equal to that block's P from a one-slot call, and those seven go through the model."""
    import torch
    from oracle import lcg_bytes
    dev = torch.device("cuda:0")
    ns, nb, bl, N = 8, 8750, 512, 256
    seven = lcg_bytes(7 * bl, 4242)[0].reshape(7, 1, bl)
    b1 = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 1)
    big = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), ns)
    idx = torch.arange(ns * nb, device=dev) % 7
    iq = torch.from_numpy(seven.reshape(7, bl)).to(dev)[idx].contiguous()
    assert iq.shape == (ns * nb, bl) and iq.dtype == torch.uint8
    for window in (WINDOW_RECT, WINDOW_HANN):
        single = np.concatenate([spectrum_dev(b1, seven[j:j + 1], N, window) for j in range(7)], axis=0)        # [7, 1, N]
        assert_rules(single, *models_of(seven, N, window), N, window, "one-slot calls, window %d" % window)
        out = torch.full((ns * nb, N), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        big.spectrum_device(iq, nb, N, out, window=window)
        big.sync()
        want = torch.from_numpy(single.reshape(7, N)).to(dev)[idx]
        wrong = (out.view(torch.int32) != want.view(torch.int32)).any(dim=1)
        assert not bool(wrong.any()), "window %d: slots that differ from the one-slot call: %s ..." % (window, wrong.nonzero().flatten()[:8].tolist())
    b1.close()
    big.close()


def test_spectrum_calls_inside_a_captured_graph(R):
    """One torch stream, no branches.  (1024, Hann) and (256, rectangular) are warmed once, then {spectrum 1024, run_device, spectrum 256,
    run_device} is captured and replayed twice with the IQ buffers refilled in between.  (Two run_device launches: the carried state is
    ping-ponged between two buffers, so a graph must hold an even number of demodulator launches to come out where it went in -
    tests/test_gpu_parity.py, test_launches_captured_in_a_hip_graph.)  The spectra are bit-equal to direct calls on a fresh batch; PCM and lens
    equal those of a batch that ran the same launches directly.  A pair never used on the batch is refused inside a capture with FMD_E_STATE;
    that capture ends normally and its graph replays."""
    import torch
    dev = torch.device("cuda:0")
    L = R.lib()
    bl, ns = 8192, 2
    cfg = R.wbfm_config(block_len=bl, **KW)
    iq_np = np.stack([iq_of("dds", 4 * bl), iq_of("lcg", 4 * bl)]).reshape(ns, 4, bl)

    def buffers(b):
        return dict(iq=[torch.zeros((ns, 1, bl), dtype=torch.uint8, device=dev) for _ in range(2)],
                    pcm=[torch.zeros((ns, 1, b.pcm_stride), dtype=torch.int16, device=dev) for _ in range(2)],
                    lens=[torch.zeros((ns, 1), dtype=torch.int32, device=dev) for _ in range(2)],
                    p1024=torch.full((ns, 1, 1024), -1.0, dtype=torch.float32, device=dev),
                    p256=torch.full((ns, 1, 256), -1.0, dtype=torch.float32, device=dev))

    def launches(b, m, st):
        b.spectrum_device(m["iq"][0], 1, 1024, m["p1024"], window=WINDOW_HANN, hip_stream=st.cuda_stream)
        b.run_device(m["iq"][0], 1, m["pcm"][0], m["lens"][0], hip_stream=st.cuda_stream)
        b.spectrum_device(m["iq"][0], 1, 256, m["p256"], window=WINDOW_RECT, hip_stream=st.cuda_stream)
        b.run_device(m["iq"][1], 1, m["pcm"][1], m["lens"][1], hip_stream=st.cuda_stream)

    def refill(m, r):
        for j in range(2):
            m["iq"][j].copy_(torch.from_numpy(np.ascontiguousarray(iq_np[:, 2 * r + j:2 * r + j + 1])))
        m["p1024"].fill_(-1.0)
        m["p256"].fill_(-1.0)
        torch.cuda.synchronize()

    def collect(m):
        torch.cuda.synchronize()
        return [x.cpu().numpy().copy() for x in (m["p1024"], m["p256"], m["pcm"][0], m["pcm"][1], m["lens"][0], m["lens"][1])]

    st = torch.cuda.Stream()
    bg, bd = R.BatchDemod(cfg, ns), R.BatchDemod(cfg, ns)
    mg, md = buffers(bg), buffers(bd)
    torch.cuda.synchronize()
    bg.spectrum_device(mg["iq"][0], 1, 1024, mg["p1024"], window=WINDOW_HANN)        # the one warm call of each pair
    bg.spectrum_device(mg["iq"][0], 1, 256, mg["p256"], window=WINDOW_RECT)
    bg.sync()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        launches(bg, mg, st)
    fresh = R.BatchDemod(cfg, ns)
    for r in range(2):
        refill(mg, r)
        g.replay()
        got = collect(mg)
        refill(md, r)
        launches(bd, md, st)
        want = collect(md)
        assert same_bits(got[0], spectrum_dev(fresh, iq_np[:, 2 * r:2 * r + 1], 1024, WINDOW_HANN)), r
        assert same_bits(got[1], spectrum_dev(fresh, iq_np[:, 2 * r:2 * r + 1], 256, WINDOW_RECT)), r
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), r
        for a, w in zip(got[2:], want[2:]):
            assert np.array_equal(a, w), r
        assert got[2].any() and got[3].any() and (got[4] > 0).all() and (got[5] > 0).all()
    assert [bytes(bg.get_state(s)) for s in range(ns)] == [bytes(bd.get_state(s)) for s in range(ns)]

    # a pair never used on this batch, inside a capture
    p4096 = torch.full((ns, 1, 4096), -1.0, dtype=torch.float32, device=dev)
    refill(mg, 0)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        rc = L.fmd_batch_spectrum_device(bg._h, C.c_void_p(mg["iq"][0].data_ptr()), 1, 4096, WINDOW_HANN, C.c_void_p(p4096.data_ptr()),
                                         C.c_void_p(st.cuda_stream))
        msg = L.fmd_last_error().decode()
        bg.spectrum_device(mg["iq"][0], 1, 1024, mg["p1024"], window=WINDOW_HANN, hip_stream=st.cuda_stream)
    assert rc == -6 and "before the capture" in msg, (rc, msg)                          # FMD_E_STATE
    g2.replay()
    torch.cuda.synchronize()
    assert same_bits(mg["p1024"].cpu().numpy(), spectrum_dev(fresh, iq_np[:, 0:1], 1024, WINDOW_HANN))
    assert bool((p4096 == -1.0).all())
    # ... and outside a capture the same pair is made and runs
    bg.spectrum_device(mg["iq"][0], 1, 4096, p4096, window=WINDOW_HANN, hip_stream=st.cuda_stream)
    st.synchronize()
    assert same_bits(p4096.cpu().numpy(), spectrum_dev(fresh, iq_np[:, 0:1], 4096, WINDOW_HANN))
    for b in (bg, bd, fresh):
        b.close()


def test_the_same_with_or_without_squelch(R):
    """Squelch on (streams 0 and 2 with a threshold no block reaches: closed from the start, lens 0, PCM zeroed; stream 1 without): the spectra are
    bit-equal to a batch without squelch, the closed blocks' spectra are delivered and pass both rules, and PCM, lens and hits are what they
    are without the spectrum calls."""
    import torch
    dev = torch.device("cuda:0")
    bl, per, launches, N = 8192, 2, 2, 1024
    kinds = ("dds", "lcg", "tone")
    cfg = R.wbfm_config(block_len=bl, **KW)
    iq_np = np.stack([iq_of(k, per * launches * bl) for k in kinds]).reshape(3, per * launches, bl)
    parts = [torch.from_numpy(np.ascontiguousarray(iq_np[:, c * per:(c + 1) * per]).reshape(-1)).to(dev) for c in range(launches)]

    def run(squelch, with_spectrum):
        b = R.BatchDemod(cfg, 3)
        if squelch:
            b.set_squelch(np.array([1e3, 0.0, 1e3], np.float32), 0)
        pcm = [torch.full((3, per, b.pcm_stride), 7, dtype=torch.int16, device=dev) for _ in range(launches)]
        lens = [torch.full((3, per), -1, dtype=torch.int32, device=dev) for _ in range(launches)]
        spec = [torch.full((3, per, N), -1.0, dtype=torch.float32, device=dev) for _ in range(2 * launches)]
        torch.cuda.synchronize()
        for c in range(launches):
            if with_spectrum:
                b.spectrum_device(parts[c], per, N, spec[2 * c])
            b.run_device(parts[c], per, pcm[c], lens[c])
            if with_spectrum:
                b.spectrum_device(parts[c], per, N, spec[2 * c + 1])
        b.sync()
        hits = [b.squelch_hits(s) for s in range(3)] if squelch else None
        b.close()
        return [x.cpu().numpy() for x in pcm], [x.cpu().numpy() for x in lens], hits, [x.cpu().numpy() for x in spec]

    p0, l0, h0, _ = run(True, False)
    p1, l1, h1, sq_spec = run(True, True)
    _, l2, _, plain_spec = run(False, True)
    assert h0 == h1 == [1, 1, 1]
    for c in range(launches):
        assert np.array_equal(l0[c], l1[c]) and np.array_equal(p0[c], p1[c]), c
        assert (l1[c][[0, 2]] == 0).all() and (l1[c][1] > 0).all() and (l2[c] > 0).all()
        assert not p1[c][[0, 2]].any() and p1[c][1].any()
        assert same_bits(sq_spec[2 * c], sq_spec[2 * c + 1])
        for j in (2 * c, 2 * c + 1):
            assert same_bits(sq_spec[j], plain_spec[j]), j
        assert_rules(sq_spec[2 * c], *models_of(iq_np[:, c * per:(c + 1) * per], N, WINDOW_HANN), N, WINDOW_HANN, "squelch on, launch %d" % c)


def test_the_host_form_between_host_runs(R):
    """spectrum_host with n_blocks 1, 4 and 1 between run_host calls on one batch (the staging buffers grow at the 4): each spectrum is bit-equal
    to the device form, and the PCM stays the oracle's bit for bit (FMD_MATH_EXACT), so the regrowth does not disturb the carried state."""
    from oracle import OracleStream
    bl, ns, N = 8192, 2, 1024
    iq_np = np.stack([iq_of("dds", 8 * bl), iq_of("lcg", 8 * bl)]).reshape(ns, 8, bl)
    b = R.BatchDemod(R.wbfm_config(block_len=bl, math=R.MATH_EXACT, **KW), ns)
    fresh = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), ns)
    oracles = [OracleStream(**KW) for _ in range(ns)]
    nxt = 0

    def demod_one():
        nonlocal nxt
        pcm, lens = b.run_host(iq_np[:, nxt:nxt + 1], 1)
        for s in range(ns):
            want = oracles[s].block(iq_np[s, nxt])
            assert lens[s, 0] == want.size and np.array_equal(pcm[s, 0, :want.size], want), (nxt, s)
        nxt += 1

    demod_one()
    for first, nb, window in ((0, 1, WINDOW_HANN), (2, 4, WINDOW_RECT), (7, 1, WINDOW_HANN)):
        part = np.ascontiguousarray(iq_np[:, first:first + nb])
        got = b.spectrum_host(part, nb, N, window)
        assert got.shape == (ns, nb, N) and same_bits(got, spectrum_dev(fresh, part, N, window)), (first, nb)
        demod_one()
    b.close()
    fresh.close()


def test_further_refusals_leave_the_batch_working(R):
    """d_power off by 4 and by 8 bytes, n_blocks 0 and -1, a NULL d_power, window -1: FMD_E_ARG each, and the batch demodulates and takes a
    spectrum afterwards as before"""
    import torch
    from oracle import OracleStream
    L = R.lib()
    dev = torch.device("cuda:0")
    bl, N = 8192, 1024
    b = R.BatchDemod(R.wbfm_config(block_len=bl, **KW), 1)
    o = OracleStream(**KW)
    blocks = iq_of("lcg", 6 * bl).reshape(6, bl)
    iq = torch.from_numpy(np.array(blocks[0])).to(dev)
    out = torch.full((N + 16,), -1.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    first = spectrum_dev(b, blocks[0].reshape(1, 1, bl), N)
    cases = [("d_power + 4", dict(off=4)), ("d_power + 8", dict(off=8)), ("n_blocks 0", dict(nb=0)), ("n_blocks -1", dict(nb=-1)),
             ("NULL d_power", dict(null=True)), ("window -1", dict(window=-1))]
    for k, (name, c) in enumerate(cases):
        d_power = None if c.get("null") else C.c_void_p(out.data_ptr() + c.get("off", 0))
        rc = L.fmd_batch_spectrum_device(b._h, C.c_void_p(iq.data_ptr()), c.get("nb", 1), N, c.get("window", WINDOW_HANN), d_power, None)
        assert rc == -1, (name, rc, L.fmd_last_error())
        b.sync()
        assert bool((out == -1.0).all()), name
        want = o.block(blocks[k])
        pcm, lens = b.run_host(blocks[k].reshape(1, 1, bl), 1)
        assert lens[0, 0] == want.size and np.array_equal(pcm[0, 0, :want.size], want), name
        assert same_bits(spectrum_dev(b, blocks[0].reshape(1, 1, bl), N), first), name
    with pytest.raises(R.FmdError):
        b.spectrum_host(blocks[:1].reshape(1, 1, bl), 1, N, window=-1)
    b.close()
