"""The stage budget rule (tests/stage_budget.py) has teeth, shown without a GPU.

Stand-ins written in numpy go through the checker the GPU test uses:

  pass   the oracle itself (e_dev = e_ref); a float32 restatement of every stage in a DIFFERENT summation order - pairwise
         sums, np.float32 throughout, the discriminator's divide replaced by a reciprocal pushed 1 ulp off, the de-emphasis
         update fused - the evidence, before any GPU run, that the factors 2 and 3 leave room for a correct implementation;
  fail   each at the stage it touches and at no earlier one: stage A with taps rounded to 18 bits (DESIGN.md section 8's own
         rejected design), stage B with 0.2446 for 0.2447 (about 0.3 LSB: invisible to max |diff| <= 1 on most inputs),
         stage D with samples rounded to 2^-16 instead of 2^-20, stage F with the carried de-emphasis state rounded to 2^-12
         between 16-frame groups.

Also here: the oracle holds the exclusion cap on every input and configuration of tests/test_gpu_stage_budget.py, and the
float64 model checks itself against the oracle's PCM.
"""
import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import chain_f64 as C64
import stage_budget as SB

BL, CONFIGS, INPUTS, input_bytes, oracle_case = SB.BL, SB.CONFIGS, SB.INPUTS, SB.input_bytes, SB.oracle_case
F32 = np.float32


# ---------------------------------------------------------------- a float32 chain in another summation order, with knobs

def pairwise(a):
    """Sum along axis 1 as a balanced tree, every add rounded to float32."""
    a = np.ascontiguousarray(a, dtype=F32)
    while a.shape[1] > 1:
        if a.shape[1] & 1:
            a = np.concatenate([a, np.zeros((a.shape[0], 1), F32)], axis=1)
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def fir32(hist, x, half_taps, size):
    """Window of step i = [hist | x][i+1 .. i+size]; symmetric pairs folded, products summed pairwise; float32."""
    w = sliding_window_view(np.concatenate([hist[1:], x]).astype(F32), size)
    half = size // 2
    p = w[:, :half] + w[:, ::-1][:, :half]
    return pairwise(p * np.asarray(half_taps, dtype=F32)[:half])


def atan2_32(y, x, c1, rcp_ulps):
    """poly_atan2 in float32 with a = min x rcp(max), the reciprocal rcp_ulps ulps above the rounded one."""
    y, x = y.astype(F32), x.astype(F32)
    ax, ay = np.abs(x), np.abs(y)
    xneg, yneg = x < 0, y < 0
    x_major = np.where(xneg, np.where(yneg, x <= y, -x >= y), np.where(yneg, x >= -y, x >= y))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = F32(1.0) / np.where(x_major, ax, ay)
        for _ in range(rcp_ulps):
            r = np.nextafter(r, F32(np.inf))
        a = np.where(x_major, ay, ax) * r
    pi, pi_2, pi_4 = F32(C64.PI), F32(C64.PI_2), F32(C64.PI_4)
    with np.errstate(invalid="ignore"):
        r0 = a * (pi_4 - (a - F32(1.0)) * (F32(c1) + F32(C64.C2) * a))
    out = np.where(xneg,
                   np.where(yneg, np.where(x_major, r0 - pi, -r0 - pi_2), np.where(x_major, -r0 + pi, pi_2 + r0)),
                   np.where(yneg, np.where(x_major, -r0, r0 - pi_2), np.where(x_major, r0, pi_2 - r0)))
    out = np.where(y == 0, np.where(xneg, pi, F32(0)), out)
    out = np.where(x == 0, np.where(yneg, -pi_2, np.where(y > 0, pi_2, F32(0))), out)
    return out.astype(F32)


def standin_trace(cfg, taps, iq, nb, fb=None, c1=0.2447, rcp_ulps=1, d_quant=None, f_state_quant=None):
    """The whole chain in float32, block by block, state carried in float32.  Knobs (the mutants): fb - other decimator taps;
    c1 - the polynomial's first coefficient; d_quant - grid the second stage's samples are rounded to; f_state_quant - grid the
    de-emphasis state is rounded to between 16-frame groups."""
    size, mode, half = int(cfg.size), int(cfg.mode), int(cfg.size) // 2
    fast, slow = int(cfg.rate_out), int(cfg.rate_out2)
    fb = np.asarray(taps["fb"] if fb is None else fb, dtype=F32)
    fm, fp, fs = (np.asarray(taps[k], dtype=F32) for k in ("fm", "fp", "fs"))
    swf, cwf = F32(taps["swf"]), F32(taps["cwf"])
    lam, coef = F32(cfg.deemph_lambda), F32(cfg.volume) * F32(32768.0)
    qd = (lambda a: a) if d_quant is None else (lambda a: (np.rint(a.astype(np.float64) / d_quant) * d_quant).astype(F32))
    tb = np.zeros(48, F32)
    pre = (F32(0), F32(0))
    br, bm, bs = np.zeros(size, F32), np.zeros(size, F32), np.zeros(size, F32)
    pp, acc = F32(0), 0
    dl = [F32(0), F32(0)]
    frames_done = 0
    trace = []
    for k in range(nb):
        # stage A
        c = np.concatenate([tb, C64.convert(iq[k * BL:(k + 1) * BL], int(cfg.offset_tuning)).astype(F32)])
        tb = c[-48:].copy()
        y = np.empty(BL // 8, F32)
        for comp in (0, 1):
            w = sliding_window_view(c[comp::2], 32)[::8][: BL // 16]
            y[comp::2] = pairwise((w[:, :16] + w[:, ::-1][:, :16]) * fb)
        # stage B
        re, im = y[0::2], y[1::2]
        pr = np.concatenate([[pre[0]], re[:-1]]).astype(F32)
        pj = np.concatenate([[pre[1]], im[:-1]]).astype(F32)
        pre = (re[-1], im[-1])
        v = atan2_32(pr * im - pj * re, re * pr + im * pj, c1, rcp_ulps)
        # stages C and D
        e, acc1 = C64.emit_steps(acc, slow, fast, v.size)
        vw = v.copy()
        if mode == 1:
            frames = fir32(qd(br), qd(vw), fm, size)[e]
        else:
            def stage_c(vv):
                vm, vp, vs = fir32(br, vv, fm, size), fir32(br, vv, fp, size), fir32(br, vv, fs, size)
                ppv = np.concatenate([[pp], vp[:-1]]).astype(F32)
                cx, cy = vp * swf, vp * cwf - ppv
                with np.errstate(divide="ignore", invalid="ignore"):
                    z = cy / cx
                    car = np.where(cx == 0, F32(0), (z + z) / (F32(1) + z * z)).astype(F32)
                return vm, vp, vs * car

            def stage_d(vm, s):
                om, os_ = fir32(qd(bm), qd(vm), fm, size)[e], fir32(qd(bs), qd(s), fm, size)[e]
                out = np.empty(2 * e.size, F32)
                out[0::2], out[1::2] = om + os_, om - os_
                return out
            vm, vp, s = stage_c(vw)
            if e.size and e[0] == 0:
                vw[1] = stage_d(vm, s)[1]
                vm, vp, s = stage_c(vw)
            frames = stage_d(vm, s)
            bm = np.concatenate([bm, vm])[-size:]
            bs = np.concatenate([bs, s])[-size:]
            pp = vp[-1]
        br = np.concatenate([br, vw])[-size:]
        acc = acc1
        # stage F: the update as one fused multiply-add (the product exact in double), then the scale
        nch = 2 if mode == 2 else 1
        t = np.empty(frames.size, F32)
        for i in range(frames.size):
            ch = i % nch
            if f_state_quant is not None and ch == 0 and frames_done % 16 == 0:
                dl = [F32(np.rint(float(d) / f_state_quant) * f_state_quant) for d in dl]
            x = frames[i]
            d = dl[ch] - x
            p = F32(float(lam) * float(d) + float(x)) if int(cfg.deemph) else x
            dl[ch] = p
            t[i] = p * coef
            if ch == nch - 1:
                frames_done += 1
        trace.append({"y": y, "v": v, "mpx": frames, "pcm": C64.to_s16(t.astype(np.float64))})
    return trace


STAGES = ("y", "v", "mpx", "pcm")


def first_failing_stage(cfg_name, inp, nb, trace, report=None):
    """Runs the checker stage by stage; returns the first stage that exceeds its budget (None: all inside)."""
    _, cfg, taps, ref = oracle_case(cfg_name, inp, nb)
    dev = SB.StageErrors(trace, input_bytes(inp, nb), BL, cfg, taps)
    dev.check_excluded_cap("%s/%s" % (cfg_name, inp))
    b_f, _ = SB.boundary_margin(ref, cfg)
    failed = None
    for st in STAGES:
        if st == "mpx" and inp == "lcg" and int(cfg.mode) == 2:
            continue                                     # noise has no pilot
        try:
            if st == "pcm":
                SB.check_pcm("%s/%s" % (cfg_name, inp), dev, b_f)
            else:
                if report is not None:
                    report.append((st, dev.err(st), ref.err(st)))
                SB.check_rule(st, "%s/%s" % (cfg_name, inp), dev.err(st), ref.err(st))
        except SB.BudgetExceeded as ex:
            print(ex)
            failed = failed or ex.stage
    return failed


CASES = [("stereo_300k", "lcg"), ("stereo_300k", "dds100"), ("stereo_300k", "dds20"), ("mono_300k", "lcg"), ("nfm_25k", "dds20")]


@pytest.mark.parametrize("cfg_name,inp", CASES)
def test_the_oracle_is_inside_its_own_budget(cfg_name, inp):
    trace, _, _, _ = oracle_case(cfg_name, inp, 2)
    assert first_failing_stage(cfg_name, inp, 2, trace) is None


@pytest.mark.parametrize("cfg_name,inp", CASES)
def test_float32_in_another_summation_order_is_inside_the_budget(cfg_name, inp):
    _, cfg, taps, _ = oracle_case(cfg_name, inp, 2)
    rep = []
    trace = standin_trace(cfg, taps, input_bytes(inp, 2), 2)
    failed = first_failing_stage(cfg_name, inp, 2, trace, rep)
    for st, d, r in rep:
        print("%s/%s %s: stand-in %r | oracle %r | x%.2f rms x%.2f max" % (cfg_name, inp, st, d, r, d.rms / max(r.rms, 1e-300), d.max / max(r.max, 1e-300)))
    assert failed is None


MUTANTS = {
    "y": lambda taps: dict(fb=SB.quantise(taps["fb"], 18)),            # stage A, 18-bit taps
    "v": lambda taps: dict(c1=0.2446),                                 # stage B, one coefficient
    "mpx": lambda taps: dict(d_quant=2.0 ** -16),                      # stage D, samples on a 2^-16 grid
    "pcm": lambda taps: dict(f_state_quant=2.0 ** -12),                # stage F, carried state on a 2^-12 grid
}


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("cfg_name,inp", [("stereo_300k", "dds100"), ("stereo_300k", "dds20"), ("mono_300k", "lcg")])
def test_a_mutant_fails_at_its_own_stage_and_at_no_earlier_one(cfg_name, inp, stage):
    _, cfg, taps, _ = oracle_case(cfg_name, inp, 2)
    trace = standin_trace(cfg, taps, input_bytes(inp, 2), 2, **MUTANTS[stage](taps))
    assert first_failing_stage(cfg_name, inp, 2, trace) == stage


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_the_oracle_holds_the_exclusion_cap(cfg_name, inp):
    """Every input and configuration of the GPU test, four blocks: the share of discriminator samples the stage-B comparison leaves
    out stays under 2e-3 of each block with the oracle's own y and v."""
    _, _, _, ref = oracle_case(cfg_name, inp, 4)
    print(cfg_name, inp, ["%.1e" % s for s in ref.excluded_share])
    ref.check_excluded_cap("%s/%s" % (cfg_name, inp))


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_model_pcm_equals_the_oracles_up_to_its_rounding(cfg_name, inp):
    """chain_f64 end to end (every stage fed by the model's own values): its rounded PCM is the oracle's except where a rounding
    boundary falls between the two t values.  The chance of that for an error e is |e|, so the share of differing values is at
    most E|e| <= rms(e); asserted at 2 rms(t_oracle - t64).  Sixteen blocks: the expected count of differing values is then 14 or
    more and the bound twice that or more, several standard deviations of the count away (four blocks expect 3 and see up to 9)."""
    nb = 16
    trace, cfg, taps, ref = oracle_case(cfg_name, inp, nb)
    _, t_o = SB.boundary_margin(ref, cfg)
    model = C64.run_chain(input_bytes(inp, nb), BL, cfg, taps)
    t64 = np.concatenate([m["t"] for m in model])
    pcm64 = np.concatenate([m["pcm"] for m in model])
    assert t64.size == t_o.size
    share = float(np.mean(pcm64 != ref.pcm))
    p = 2.0 * SB.rms(t_o - t64)
    print("%s/%s: PCM differs on %.2e of %d values; rms(t_oracle - t64) %.3e LSB" % (cfg_name, inp, share, t64.size, SB.rms(t_o - t64)))
    assert share <= p


def test_fixed_point_fir_restates_the_documented_form():
    """stage_budget.fixed_point_fir: with all nine limb pairs it IS the filter of the rounded taps over the rounded samples; with
    six the difference stays inside section 2a's bound for the pairs left out, c0 2^-24 128 sum(|t1| + |t2|) + c0 2^-32 128 sum|t2|."""
    _, cfg, taps, _ = oracle_case("stereo_300k", "dds100", 2)
    rng = np.random.default_rng(7)
    x, hist = rng.uniform(-3.1, 3.1, 4096), rng.uniform(-3.1, 3.1, 90)
    for k in ("fm", "fp", "fs"):
        h = C64.full_taps(taps[k], 90)
        qf = SB.taps_qf(h)
        hq = SB.quantise(h, qf)
        want = C64._fir(np.rint(hist * 2.0 ** 20) / 2.0 ** 20, np.rint(x * 2.0 ** 20) / 2.0 ** 20, hq)
        nine = SB.fixed_point_fir(hist, x, h, pairs=9)
        assert np.abs(nine - want).max() < 1e-13, k
        t = SB.limbs(hq * 2.0 ** qf)
        bound = 2.0 ** (12 - qf) * (2.0 ** -24 * 128 * (np.abs(t[1]).sum() + np.abs(t[2]).sum()) + 2.0 ** -32 * 128 * np.abs(t[2]).sum())
        six = SB.fixed_point_fir(hist, x, h)
        assert 0 < np.abs(six - nine).max() <= bound, (k, np.abs(six - nine).max(), bound)
