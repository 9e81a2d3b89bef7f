"""The RDS receiver without a device (include/fmdemod_mi355x.h, "RDS receiver"): the block / group decoder of csrc/fmd_rds.c
against synthesised bit streams, the float64 model end to end from a synthesised multiplex (MPX -> subc_model -> rds_model -> decoder) at the three
rates, with and without a clock offset, the teeth of the bounds the GPU tests hold the kernels to - at the shapes of tests/test_gpu_rds.py and at
the edge shapes of tests/test_gpu_rds_edges.py (rds_model.EDGE_SHAPES), where a slicer that stops at 256 bits, a dropped chunk partial and a y history
cut to 64 values are planted too - and csrc/fmd_rds.c under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
(tests/c/rds_check.c).

Garbage and acquisition.  Two valid remainders 26 bits apart in cyclic order is the acquisition rule; on random bits a given bit completes such
a pair with probability 6 / 1024^2: 0.57 expected acquisitions in 10^5 bits.  The 10^5 bits of numpy's default_rng(0) hold none - a property of
that fixed stream, not of the rule; the test beside it counts what ten such streams do (DESIGN.md section 5d states the limit)."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rds_model as RM  # noqa: E402
import subc_model as SM  # noqa: E402

import rtl_fm_player_amd as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")

#                (rate_z, Tg, Bz): the shapes of tests/test_gpu_rds.py
GPU_SHAPES = [(18750, 64, 64), (12000, 16, 112), (15000, 48, 256), (18750, 64, 1024), (18750, 64, 1280)]
#                ... and of tests/test_gpu_rds_edges.py
EDGE_SHAPES = [shape for shape, _, _ in RM.EDGE_SHAPES]


@pytest.fixture(scope="module", autouse=True)
def built():
    R.build_library()


groups_of = RM.groups_of


def full_groups(got):
    return [g[:4] for g in got if g[4] == 15]


# ---- 1. the decoder ----------------------------------------------------------------------------------------------------------------------------

def test_every_split_of_the_push_gives_the_same_groups():
    groups = groups_of(12)
    soft = RM.soft_of_bits(RM.data_bits(groups))
    whole = R.RdsDecoder().push(soft)
    assert full_groups(whole) == groups and [g[5] for g in whole] == [0] * 12
    rng = np.random.default_rng(3)
    for trial in range(12):
        dec, got, at = R.RdsDecoder(), [], 0
        while at < soft.size:
            n = 1 if trial == 0 else int(rng.integers(1, 1 + (7, 26, 104, 300)[trial % 4]))
            got += dec.push(soft[at:at + n])
            at += n
        assert got == whole, trial
    # the amplitude does not matter, only the sign; a version-B group carries C'
    assert R.RdsDecoder().push(soft * 1e-20) == whole
    gb = RM.ps_groups(0xBEEF, "VERSIONB", n=6, version_b=True)
    got = R.RdsDecoder().push(RM.soft_of_bits(RM.data_bits(gb, version_b=True)))
    assert full_groups(got) == gb and [g[5] for g in got] == [1] * 6
    # ... and C where C' belongs marks the block bad
    mixed = RM.soft_of_bits(np.concatenate([RM.data_bits(gb[:2], True), RM.data_bits(gb[2:3], False), RM.data_bits(gb[3:], True)]))
    assert [g[4] for g in R.RdsDecoder().push(mixed)] == [15, 15, 11, 15, 15, 15]


def test_one_flipped_bit_marks_its_block_bad_and_no_wrong_group_comes_out():
    groups = groups_of(16)
    bits = RM.data_bits(groups)
    rng = np.random.default_rng(4)
    for g in range(2, 16):                                   # (the first two groups: acquisition)
        bits[104 * g + 26 * (g & 3) + int(rng.integers(26))] ^= 1
    dec = R.RdsDecoder()
    got = dec.push(RM.soft_of_bits(bits))
    assert len(got) == 16 and dec.dec.n_loss == 0
    for g in range(2, 16):
        assert got[g][4] == 15 & ~(1 << (g & 3)), g
        assert all(got[g][p] == groups[g][p] for p in range(4) if got[g][4] & (1 << p))
    assert full_groups(got) == groups[:2]


def test_garbage_never_syncs():
    bits = np.random.default_rng(0).integers(0, 2, 100000)
    dec = R.RdsDecoder()
    assert dec.push(RM.soft_of_bits(bits)) == [] and dec.dec.n_sync == 0 and not dec.synced and dec.dec.bits == 100000
    assert dec.pi is None and dec.ps == ""


def test_false_acquisitions_on_garbage_are_as_rare_as_the_rule_says_and_never_last():
    """10^6 random bits (ten seeds): the rule expects 6 / 1024^2 per bit = 5.7 acquisitions; more than 14 has a Poisson probability below 0.1 %.
    Each is dropped again after FMD_RDS_SYNC_LOSS bad blocks, and all that comes out of it is one group with the two acquisition blocks marked."""
    n_sync, masks = 0, []
    for seed in range(10):
        dec = R.RdsDecoder()
        got = dec.push(RM.soft_of_bits(np.random.default_rng(seed).integers(0, 2, 100000)))
        assert dec.dec.n_loss == dec.dec.n_sync and not dec.synced
        n_sync += dec.dec.n_sync
        masks += [g[4] for g in got]
    print("%d false acquisitions in 10^6 random bits, masks %s" % (n_sync, masks))
    assert n_sync <= 14 and len(masks) <= n_sync and all(bin(m).count("1") <= 2 for m in masks)


def test_resync_after_a_dropped_bit():
    groups = groups_of(20)
    bits = np.delete(RM.data_bits(groups), 104 * 8 + 37)
    dec = R.RdsDecoder()
    got = dec.push(RM.soft_of_bits(bits))
    assert (dec.dec.n_sync, dec.dec.n_loss, dec.synced) == (2, 1, True)
    full = full_groups(got)
    # the group of the drop, FMD_RDS_SYNC_LOSS = 6 bad blocks and two blocks to acquire again: at most four groups are lost
    assert full[:8] == groups[:8] and full[8:] == groups[20 - len(full[8:]):] and len(full) >= 16
    for g in got:                                            # whatever came out marked ok was sent
        assert any(all(g[p] == s[p] for p in range(4) if g[4] & (1 << p)) for s in groups)


def test_ps_name_pi_and_pty_from_0a_groups():
    dec = R.RdsDecoder()
    dec.push(RM.soft_of_bits(RM.data_bits(RM.ps_groups(0xD3A5, "HELLO FM", pty=5, n=2))))
    assert dec.pi == 0xD3A5 and dec.pty == 5 and dec.ps == "HELL    "
    dec.push(RM.soft_of_bits(RM.data_bits(RM.ps_groups(0xD3A5, "HELLO FM", pty=5, n=4)[2:])))
    assert dec.ps == "HELLO FM" and dec.info.ps_mask == 15
    # a group type other than 0 leaves the name alone; a block not ok is not taken
    L = R.lib()
    import ctypes as C
    g = R.FmdRdsGroup((0x1111, 0x2000 | (7 << 5), 0x5858, 0x5858), 15, 0)
    L.fmd_rds_info_update(C.byref(dec.info), C.byref(g))
    assert dec.ps == "HELLO FM" and dec.pi == 0x1111 and dec.pty == 7
    g = R.FmdRdsGroup((0x2222, (3 << 5) | 1, 0, 0x5858), 0b0110, 0)
    L.fmd_rds_info_update(C.byref(dec.info), C.byref(g))
    assert dec.ps == "HELLO FM" and dec.pi == 0x1111 and dec.pty == 3


def test_design_table_and_range_of_the_library_are_the_models():
    for rate_z, Tg, Bz in GPU_SHAPES:
        cfg = R.FmdRdsConfig(rate_z, Bz, Tg, 8, 4)
        want = RM.design(rate_z, Tg)
        got = R.rds_design(cfg)
        assert np.abs(got - want).max() <= 2 * RM.U * np.abs(want).max()
        # an ideal isolated bit reads 1 at its centre
        k = np.arange(Tg)
        assert abs(np.dot(want, RM.pulse(((Tg - 1) / 2.0 - k) * RM.FB / rate_z)) - 1) < 1e-12
    geo = RM.Geometry(18750, 1024)
    assert (geo.pw, geo.hh, geo.lb, geo.hb, geo.hy, geo.slot) == (300, 8, 10, 16, 34, 68)
    assert [round(2 * r / 2375, 2) for r in (18750, 15000, 12000)] == [15.79, 12.63, 10.11]
    import ctypes as C
    L = R.lib()
    taps = np.zeros(64, dtype=np.float32)
    for bad in ((18750, 62, 64, 8, 4), (18751, 64, 64, 8, 4), (9000, 64, 16, 8, 4), (40000, 256, 64, 8, 4), (18750, 32, 16, 8, 4), (18750, 64, 68, 8, 4),
                (18750, 64, 64, 0, 4), (18750, 64, 64, 8, 0)):
        cfg = R.FmdRdsConfig(*bad)
        assert L.fmd_rds_design(C.byref(cfg), taps.ctypes.data) == -2, bad


# ---- 2. end to end in the float64 model ----------------------------------------------------------------------------------------------------------

def model_chain(rate, D, M, Tg, groups, ppm=0.0, t0=3.0, level=0.04, avg=8, dtype=np.float64):
    bits = RM.data_bits(groups)
    n = int(len(bits) * rate / RM.FB) + 4 * M
    n -= n % M
    v = RM.mpx(bits, rate, n, level=level, t0=t0, ppm=ppm)
    z, _ = SM.subc_f64(v, SM.design(rate, 2400, 128).astype(np.float32), rate, 57000, D)
    geo = RM.Geometry(rate // D, M // D)
    out, _ = RM.receive(z, geo, RM.design(rate // D, Tg).astype(np.float32), avg, dtype=dtype)
    return out


@pytest.mark.parametrize("rate,Tg", [(300000, 64), (240000, 48), (192000, 40)])
def test_end_to_end_in_the_float64_model(rate, Tg):
    """MPX (RDS at 0.04 beside a pilot of 0.157 and a 1 kHz tone of 0.3) -> subcarrier receiver (57 kHz, 2.4 kHz, 128 taps, D 16) -> RDS receiver
    (avg_blocks 8) -> decoder: every group but the first 3 comes out, in order, all four blocks ok, none wrong"""
    groups = groups_of(12)
    out = model_chain(rate, 16, 16384, Tg, groups)
    assert out["counts"].sum() == -(-RM.Q * (out["y"].size - RM.Geometry(rate // 16, 1024).lb) // (2 * rate // 16))        # the nominal count
    dec = R.RdsDecoder()
    got = dec.push(np.concatenate(out["soft"]))
    full = full_groups(got)
    print("rate %d: %d groups out, %d whole, the first whole one is sent group %d" % (rate, len(got), len(full), groups.index(full[0])))
    assert all(g in groups for g in full) and full == groups[12 - len(full):] and len(full) >= 9
    assert dec.ps == "RADIO 42" and dec.pi == 0x1234


def test_end_to_end_with_a_clock_offset_of_50_ppm_across_one_wrap_of_phi():
    """+50 ppm: phi drifts by 50e-6 bit per bit (a full turn in 20 000 bits, 17 s).  The span starts at phi = 0.45 and holds one wrap to -1/2, where
    one bit is read twice: the decoder loses sync (6 bad blocks) and acquires again (2 blocks).  Window: the group of the wrap, the one before it
    and three after it; every other group but the first 3 decodes."""
    groups = groups_of(26)
    out = model_chain(300000, 16, 16384, 64, groups, ppm=50.0, t0=3.26)
    phi = out["phi"]
    wraps = [b for b in range(1, phi.size) if abs(phi[b] - phi[b - 1]) > 0.5]
    assert len(wraps) == 1 and 0.44 < phi[0] < 0.46 and phi[wraps[0] - 1] > 0.49 and phi[wraps[0]] < -0.49, phi
    gw = int(out["first"][wraps[0]]) // 104
    dec = R.RdsDecoder()
    full = full_groups(dec.push(np.concatenate(out["soft"])))
    lost = [i for i, g in enumerate(groups) if g not in full]
    print("wrap in block %d (group %d); groups not whole: %s" % (wraps[0], gw, lost))
    assert all(g in groups for g in full) and [groups.index(g) for g in full] == sorted(groups.index(g) for g in full)
    assert all(i < 3 or gw - 1 <= i <= gw + 3 for i in lost), (gw, lost)
    assert dec.dec.n_sync >= 2


# ---- 3. teeth: what the bounds of the GPU tests catch ---------------------------------------------------------------------------------------------

def bounds_of(z, geo, taps, out64):
    """(y bound re, im; Tm bound per block; soft bound per block with the model's own phi) for one stream from reset"""
    T = len(taps)
    br, bi = RM.y_bound(z, taps, np.zeros(T))
    bt = RM.tm_bound(out64["y"], br, bi, geo.bz)
    yext = np.concatenate([np.zeros(geo.hy), out64["y"]])
    byext = np.concatenate([np.zeros(geo.hy), np.maximum(br, bi)])
    es, counts, _ = RM.block_counts(geo, RM.Q * geo.lb, z.size // geo.bz)
    bs = []
    for b in range(z.size // geo.bz):
        lo = b * geo.bz
        bs.append(RM.soft_bound(geo, yext[lo:lo + geo.hy + geo.bz], byext[lo:lo + geo.hy + geo.bz], es[b], counts[b], out64["phi"][b]))
    return br, bi, bt, bs


def shares(out, out64, bounds):
    br, bi, bt, bs = bounds
    ey = out["y"].astype(np.complex128) - out64["y"]
    et = out["tm"].astype(np.complex128) - out64["tm"]
    sy = max((np.abs(ey.real) / br).max(), (np.abs(ey.imag) / bi).max())
    st = max((np.abs(et.real) / bt).max(), (np.abs(et.imag) / bt).max())
    ss = max([0.0] + [float((np.abs(a.astype(np.float64) - b) / c).max()) for a, b, c in zip(out["soft"], out64["soft"], bs) if len(a) and len(a) == len(b)])
    return sy, st, ss


@pytest.mark.parametrize("shape", GPU_SHAPES + EDGE_SHAPES)
def test_the_bounds_hold_the_float32_model_and_catch_every_planted_defect(shape):
    """On each GPU shape, LCG input, 4 blocks from reset.  The float32 model (unfused, sequential sums; sliced with the float64 model's phi) stays
    inside the bounds of y, Tm and the soft bits.  Each defect, planted into the float64 model, exceeds the bound of what it touches by a factor
    of more than 50 (the figures per shape are printed, and recorded in DESIGN.md section 5d):
      one tap zeroed (y); the z history one sample late at block 1's edge (y); the table index held across block 1 (Tm); s(k-1) of block 2's first
      bit from block 1's phi (soft bits); ownership off by one bit at block 2's edge (first index and count - integers - and the soft bits)."""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    taps = RM.design(rate_z, Tg).astype(np.float32)
    z = RM.lcg_complex(4 * Bz, 77)
    out64, _ = RM.receive(z, geo, taps)
    bounds = bounds_of(z, geo, taps, out64)
    out32, _ = RM.receive(z, geo, taps, dtype=np.float32, phi_given=out64["phi"])
    sy, st, ss = shares(out32, out64, bounds)
    print("shape %s: the float32 model uses %.4f (y) %.4f (Tm) %.4f (soft) of the bounds" % (shape, sy, st, ss))
    assert max(sy, st, ss) < 1
    assert np.array_equal(out32["counts"], out64["counts"]) and np.array_equal(out32["first"], out64["first"])
    factor = {}
    for name, mut, pick in (("tap zeroed", {"zero_tap": Tg // 2 - 3}, 0), ("history late", {"late_history": 1}, 0), ("w index held", {"held_w": 1}, 1),
                            ("wrong block's phi", {"wrong_phi": 2}, 2), ("ownership off by one", {"own_off": 2}, 2)):
        bad, _ = RM.receive(z, geo, taps, mutate=mut, phi_given=out64["phi"])
        if name == "ownership off by one":
            assert bad["first"][2] == out64["first"][2] and bad["counts"][2] == out64["counts"][2] - 1 and bad["first"][3] == out64["first"][3] - 1
            n = len(bad["soft"][2])
            factor[name] = float((np.abs(bad["soft"][2] - out64["soft"][2][:n]) / bounds[3][2][:n]).max())
        else:
            factor[name] = shares(bad, out64, bounds)[pick]
    print("shape %s: defects exceed their bounds by %s" % (shape, {k: "%.3g" % v for k, v in factor.items()}))
    if Bz % geo.pw == 0:                                    # (a block of whole timing periods - Pw = 32, Bz = 65536: holding the index is no fault, nothing to plant)
        assert factor.pop("w index held") == 0
    assert min(factor.values()) > 50, factor


@pytest.mark.parametrize("shape,nb,S", [e for e in RM.EDGE_SHAPES if e[0][2] >= 2600])
def test_a_slicer_that_stops_at_256_bits_or_a_dropped_chunk_partial_cannot_pass(shape, nb, S):
    """What the GPU tests of the blocks of more than 256 bits and more than 2 chunks rest on, in the float64 model on the LCG input of seed 77, which
    tests/test_gpu_rds_edges.py feeds stream 0 at the edge shapes' block counts.
    A slicer whose loop ended after one trip would leave +0 in the bits j >= 256 of a block: at (11875, 16, 2816) and (12000, 32, 4096) every
    one of them (25 / 26 / 26 and 149 / 149 / 150) has |c_j| > 50 x its soft_bound - the smallest ratio is 93 - so a zero there cannot pass.
    (At Bz = 65536 some of the 1800 to 3900 such bits of a block are small by chance; most of them are not.)
    A tracker that dropped a block's last chunk partial would miss that chunk's part of Tm and of sum p: the larger component of the first and
    the second exceed 10 x tm_bound in every block (Tm 429 to 1657 x at 3 and 4 chunks, 13 x to 34 x at 64 chunks; sum p above 340 x)."""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    taps = RM.design(rate_z, Tg).astype(np.float32)
    chunk0 = (-(-Bz // 1024) - 1) * 1024                    # the last chunk's first sample
    assert chunk0 >= 2048
    z = RM.lcg_complex(nb * Bz, 77)
    out, _ = RM.receive(z, geo, taps)
    _, _, bt, bs = bounds_of(z, geo, taps, out)
    y = out["y"].reshape(nb, Bz)
    low_soft, low_tm, low_pw, n_late = [], [], [], []
    for b in range(nb):
        assert out["counts"][b] > 256
        ratio = np.abs(out["soft"][b][256:]) / bs[b][256:]
        low_soft.append(float(ratio.min()))
        n_late.append(int((ratio > 50).sum()))
        p = np.abs(y[b, chunk0:]) ** 2
        part = np.sum(p * RM.table_exact(geo, (b * Bz + chunk0 + np.arange(Bz - chunk0)) % geo.pw))
        low_tm.append(max(abs(part.real), abs(part.imag)) / bt[b])
        low_pw.append(p.sum() / bt[b])
    print("shape %s: bits past 256 with |c| > 50 x bound per block %s of %s, smallest |c| / bound %.3g; the last chunk's part of Tm %s x tm_bound, of sum p "
          "at least %.0f x" % (shape, n_late, [int(c) - 256 for c in out["counts"]], min(low_soft), ["%.0f" % v for v in low_tm], min(low_pw)))
    if Bz < 65536:
        assert n_late == [int(c) - 256 for c in out["counts"]] and min(low_soft) > 50
    else:
        assert min(n_late) > 1000
    assert min(low_tm) > 10 and min(low_pw) > 10


@pytest.mark.parametrize("shape,nb,S", [e for e in RM.EDGE_SHAPES if RM.Geometry(e[0][0], e[0][2]).hy > 64 and e[1] > 2])
def test_a_state_that_carries_64_of_the_66_lookback_values_cannot_pass(shape, nb, S):
    """Hy = 66 at S = 32 is more than the 64 samples the matched filter stages.  Single-block launches on the GPU tests' synthesised input, the
    newest two values of the carried y history lost (zero) at every hand-over, in the float64 model: some block's first bits move by more than
    50 x their soft_bound, so the bit equality of the split runs cannot hold.  (With the one hand-over of the 2-block shape at Bz = 65536 no bit
    happens to read those two values; there the GPU test compares the carried history itself.)"""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    taps = RM.design(rate_z, Tg).astype(np.float32)
    z = RM.synth_z(rate_z, S, nb * Bz, max(4, RM.groups_to_fill(rate_z, nb * Bz)))[0]
    out, _ = RM.receive(z, geo, taps)
    _, _, _, bs = bounds_of(z, geo, taps, out)
    st, worst = None, 0.0
    for b in range(nb):
        if st is not None:
            st.yhist = st.yhist.copy()
            st.yhist[64:] = 0
        o, st = RM.receive(z[b * Bz:(b + 1) * Bz], geo, taps, state=st, phi_given=out["phi"][b:b + 1])
        if len(bs[b]):
            worst = max(worst, float((np.abs(o["soft"][0] - out["soft"][b]) / bs[b]).max()))
    print("shape %s: soft bits move by up to %.3g x their bound" % (shape, worst))
    assert worst > 50


@pytest.mark.parametrize("shape,nb,S", [e for e in RM.EDGE_SHAPES if e[1] > 2])
def test_the_synthesised_input_leaves_enough_blocks_for_the_phi_rule(shape, nb, S):
    """DESIGN.md section 2b's rule is applied to phi over the blocks whose |Ts| exceeds a quarter of the stream's largest; the GPU test asks for six
    of them over its streams.  In the float64 model, on the input it uses, at its block counts: 20, 25, 18, 9 and 9."""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    z = RM.synth_z(rate_z, S, nb * Bz, max(4, RM.groups_to_fill(rate_z, nb * Bz)))
    keep = 0
    for s in range(S):
        mag = np.abs(RM.receive(z[s], geo, RM.design(rate_z, Tg).astype(np.float32))[0]["ts"])
        keep += int((mag > 0.25 * mag.max()).sum())
    print("shape %s, %d streams x %d blocks: %d blocks with |Ts| above a quarter of the largest" % (shape, S, nb, keep))
    assert keep >= 6


# ---- 4. csrc/fmd_rds.c under the sanitizers, as a stand-alone program ------------------------------------------------------------------------------

def test_fmd_rds_c_under_asan_and_ubsan():
    tmp = tempfile.mkdtemp(prefix="fmd_rds_")
    try:
        exe = os.path.join(tmp, "rds_check")
        subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "c", "rds_check.c"), os.path.join(CSRC, "fmd_rds.c"), "-lm"], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")     # (the leak checker needs ptrace, which not every sandbox grants)
        p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        print(p.stdout)
        assert p.returncode == 0 and not p.stderr and "0 checks failed" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
