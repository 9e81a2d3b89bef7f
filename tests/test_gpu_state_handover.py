"""fmd_batch_set_state: the state struct is ALL a stream carries (include/fmdemod_mi355x.h).

A stream's state taken out of one batch with fmd_batch_get_state and put into another with fmd_batch_set_state must continue as
if nothing had happened - for every kernel family, also FMD_MATH_FAST_MFMA_F, whose launch starts from a bm ring it did not make
(lr_head_fix) - and so must the reference's own state (the oracle's), handed to the device in the middle of a run.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import BL, CONFIGS, gpu_run

pytestmark = pytest.mark.gpu

NAMES = ["stereo_300k", "mono_300k", "nfm_25k"]
FAMILIES = ["exact", "valu", "mfma", "mfma_f"]
STATE_FIELDS = ("tb", "pre_r", "pre_j", "pp", "deemph_l", "deemph_r", "acc", "br", "bm", "bs")


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def math_of(R, family):
    return {"exact": R.MATH_EXACT, "valu": R.MATH_FAST_VALU, "mfma": R.MATH_FAST_MFMA, "mfma_f": R.MATH_FAST_MFMA_F}[family]


def stream_bytes(stream, nb):
    from oracle import lcg_bytes
    return lcg_bytes(nb * BL, 12345 + stream)[0]


def run_blocks(b, iq, nb):
    """nb blocks of a 1-stream batch in one launch: (pcm concatenated, lens)."""
    out, lens = b.run_host_concat(np.ascontiguousarray(iq).reshape(1, nb, BL), nb)
    return out[0], lens[0]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", NAMES)
def test_round_trip_into_a_fresh_batch(R, name, family):
    """3 blocks on stream 5 of an 8-stream batch, get_state, set_state into stream 0 of a fresh 1-stream batch, 3 more blocks: PCM,
    lengths and the final state are those of 6 blocks run by that family without the hand-over - in one launch, and in two."""
    math = math_of(R, family)
    ns, src = 8, 5
    iq5 = stream_bytes(src, 6)
    first = np.stack([stream_bytes(s, 6)[: 3 * BL] for s in range(ns)])
    a = R.BatchDemod(R.wbfm_config(math=math, **CONFIGS[name]), ns)
    out_a, lens_a = a.run_host_concat(first.reshape(ns, 3, BL), 3)
    st = a.get_state(src)
    a.close()
    b = R.BatchDemod(R.wbfm_config(math=math, **CONFIGS[name]), 1)
    assert b.math == a.math
    b.set_state(0, st)
    assert bytes(b.get_state(0)) == bytes(st)
    out_b, lens_b = run_blocks(b, iq5[3 * BL:], 3)
    got = np.concatenate([out_a[src], out_b])
    got_lens = np.concatenate([lens_a[src], lens_b])
    got_state = bytes(b.get_state(0))
    b.close()
    for launches in (1, 2):
        want, wlens, w = gpu_run(R, CONFIGS[name], iq5, 6, math, launches=launches)
        assert np.array_equal(got_lens, wlens[0]), launches
        bad = np.flatnonzero(got != want[0])
        assert bad.size == 0, "%d launch(es): first difference at %d of %d (hand-over at %d)" % (launches, bad[0], got.size, out_a[src].size)
        assert got_state == bytes(w.get_state(0)), "%d launch(es): the final state differs" % launches
        w.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", NAMES)
def test_continues_from_the_reference_state(R, name, family):
    """The oracle runs 3 blocks; its state goes through set_state; the device runs blocks 4 - 6: exact kernels bit for bit the
    oracle's, every +-1 LSB family within one step and with the oracle's lengths."""
    from oracle import OracleStream
    iq = stream_bytes(0, 6)
    s = OracleStream(**CONFIGS[name])
    s.run(iq[: 3 * BL], BL)
    o = s.get_state()
    want, wlens = s.run(iq[3 * BL:], BL)
    from rtl_fm_player_amd.capi import FmdStreamState
    st = FmdStreamState()
    for f in STATE_FIELDS:
        setattr(st, f, getattr(o, f))
    b = R.BatchDemod(R.wbfm_config(math=math_of(R, family), **CONFIGS[name]), 1)
    b.set_state(0, st)
    got, lens = run_blocks(b, iq[3 * BL:], 3)
    b.close()
    assert np.array_equal(lens, wlens)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    tol = 0 if family == "exact" else 1
    assert d.max() <= tol, "max |diff| %d at %d (%d values differ)" % (d.max(), int(d.argmax()), int((d > tol).sum()))


def test_set_state_leaves_the_other_streams_alone(R):
    ns = 4
    iq = np.stack([stream_bytes(s, 1) for s in range(ns)])
    b = R.BatchDemod(R.wbfm_config(math=R.MATH_EXACT, **CONFIGS["stereo_300k"]), ns)
    b.run_host(iq.reshape(ns, 1, BL), 1)
    before = [bytes(b.get_state(s)) for s in range(ns)]
    assert len(set(before)) == ns                       # four different inputs: four different states
    st = b.get_state(1)
    st.pre_r, st.acc = 0.25, 7
    st.br[3] = -1.5
    b.set_state(2, st)
    after = [bytes(b.get_state(s)) for s in range(ns)]
    assert after[2] == bytes(st)
    for s in (0, 1, 3):
        assert after[s] == before[s], s
    b.close()


def test_set_state_rejects_bad_arguments(R):
    from rtl_fm_player_amd.capi import lib
    ns = 2
    b = R.BatchDemod(R.wbfm_config(math=R.MATH_EXACT, **CONFIGS["stereo_300k"]), ns)
    st = b.get_state(0)
    L = lib()
    FMD_E_ARG = -1
    assert L.fmd_batch_set_state(b._h, 0, None) == FMD_E_ARG
    assert L.fmd_batch_set_state(None, 0, C.byref(st)) == FMD_E_ARG
    for stream in (-1, ns, ns + 100):
        assert L.fmd_batch_set_state(b._h, stream, C.byref(st)) == FMD_E_ARG, stream
    assert L.fmd_batch_set_state(b._h, ns - 1, C.byref(st)) == 0
    b.close()
