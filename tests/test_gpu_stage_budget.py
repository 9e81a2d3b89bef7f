"""Per-stage error budget of the +-1 LSB kernel families against the float64 model (tests/chain_f64.py, tests/stage_budget.py).

The end-to-end tests see one observable, the int16 PCM within one step: 7.6e-5 of the signal at volume 0.4, three orders of
magnitude above the reference's own float32 rounding of a stage.  Here every stage tap of a fast kernel (fmd_debug_taps: y, v,
mpx) is held to  rms <= 2 rms(e_ref) + D,  max <= 3 max(e_ref) + D  against the float64 stage applied to the upstream values the
kernel itself produced, e_ref being the oracle's error on the same input and D derived from the documented fixed-point forms
(stage_budget.py); the PCM to round(t) of the float64 last stage over the kernel's own mpx, except within B_F of a rounding
boundary.  A failure names the stage, the family, the configuration and input, both errors and the worst sample.
"""
import numpy as np
import pytest

import stage_budget as SB
from stage_budget import BL, CONFIGS, INPUTS

pytestmark = pytest.mark.gpu

NB = 4
FAMILY = {2: "valu", 3: "mfma", 7: "mfma_f"}


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def device_trace(R, cfg_name, inp, math, time_split):
    """One launch of NB blocks with every stage tap; returns (trace, config, taps, the family that ran)."""
    import torch
    cfg = R.wbfm_config(math=math, **CONFIGS[cfg_name])
    b = R.BatchDemod(cfg, 1)
    b.set_time_split(time_split)
    M = BL // 16
    dev = torch.device("cuda:0")
    iq = torch.from_numpy(SB.input_bytes(inp, NB).copy()).to(dev)
    pcm = torch.zeros(NB * b.pcm_stride, dtype=torch.int16, device=dev)
    lens = torch.zeros(NB, dtype=torch.int32, device=dev)
    y = torch.zeros(NB * 2 * M, dtype=torch.float32, device=dev)
    v = torch.zeros(NB * M, dtype=torch.float32, device=dev)
    mpx = torch.zeros(NB * M, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    b.run_device(iq, NB, pcm, lens, debug={"y": y, "v": v, "mpx": mpx})
    b.sync()
    torch.cuda.synchronize()
    y, v, mpx, pcm, lens = (t.cpu().numpy() for t in (y, v, mpx, pcm, lens))
    trace = []
    for k in range(NB):
        n = int(lens[k])
        trace.append({"y": y[k * 2 * M:(k + 1) * 2 * M], "v": v[k * M:(k + 1) * M], "mpx": mpx[k * M:k * M + n],
                      "pcm": pcm[k * b.pcm_stride:k * b.pcm_stride + n]})
    t = R.design_taps(cfg)
    half = cfg.size // 2
    taps = {"fb": np.array(t.fb, dtype=np.float32), "fm": np.array(t.fm[:half], dtype=np.float32), "fp": np.array(t.fp[:half], dtype=np.float32),
            "fs": np.array(t.fs[:half], dtype=np.float32), "swf": t.swf, "cwf": t.cwf}
    family = b.math
    b.close()
    return trace, cfg, taps, family


@pytest.mark.parametrize("time_split", [0, 48])
@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
def test_every_stage_inside_its_budget(R, fast_math, cfg_name, inp, time_split):
    otrace, ocfg, otaps, ref = SB.oracle_case(cfg_name, inp, NB)
    trace, cfg, taps, family = device_trace(R, cfg_name, inp, fast_math, time_split)
    label = "%s/%s/%s/split%d" % (FAMILY[family], cfg_name, inp, time_split)
    iq = SB.input_bytes(inp, NB)
    assert [t["pcm"].size for t in trace] == [t["pcm"].size for t in otrace], label
    dev = SB.StageErrors(trace, iq, BL, cfg, taps)
    M = BL // 16

    # the derived terms (stage_budget.py's head): zero unless the family's documented fixed-point form says otherwise
    D = {"y": (0.0, 0.0), "v": (0.0, 0.0), "mpx": (0.0, 0.0)}
    if family in (R.MATH_FAST_MFMA, R.MATH_FAST_MFMA_F):
        D["y"] = SB.d_decimator_taps(iq, cfg, taps)                      # taps T = round(fb 2^26)
    if family == R.MATH_FAST_MFMA_F:
        d2 = SB.d_second_stage(R.config_error_estimate(cfg), cfg.volume)  # samples 2^-20, taps 2^-qf, dropped limb pairs
        dc = SB.d_stage_c_fixed_point([t["v"] for t in trace], cfg, taps)  # pilot and L-R filters: samples 2^-20, taps 2^-qf, six limb pairs
        D["mpx"] = (d2[0] + dc[0], d2[1] + dc[1])

    failures = []
    try:
        dev.check_excluded_cap(label)
    except AssertionError as ex:
        failures.append(str(ex))
    stereo_noise = inp == "lcg" and cfg.mode == 2                       # no pilot: the regenerated carrier is ill-conditioned in any arithmetic
    for st in ("y", "v", "mpx"):
        e_dev, e_ref = dev.err(st), ref.err(st)
        print("BUDGET %s %s e_dev rms %.3e max %.3e at %d | e_ref rms %.3e max %.3e | D rms %.3e max %.3e%s" %
              (label, st, e_dev.rms, e_dev.max, e_dev.worst, e_ref.rms, e_ref.max, D[st][0], D[st][1], " (not asserted)" if st == "mpx" and stereo_noise else ""))
        if st == "mpx" and stereo_noise:
            continue
        try:
            SB.check_rule(st, label, e_dev, e_ref, *D[st])
        except SB.BudgetExceeded as ex:
            failures.append(str(ex))
    b_f, t_o = SB.boundary_margin(ref, ocfg)
    print("BUDGET %s pcm B_F %.3e LSB, excluded share %s" % (label, b_f, ["%.1e" % s for s in dev.excluded_share]))
    try:
        SB.check_pcm(label, dev, b_f)
    except SB.BudgetExceeded as ex:
        failures.append(str(ex))

    # PCM against the oracle's, from the same launch.  A value differs when a rounding boundary falls between the two t: for an
    # error e the chance is |e|, so the share of differing values is at most E|e| <= rms(e) <= the stage budgets added up in PCM
    # steps (each stage's rms budget times what the float64 model downstream of it makes of a unit of error, lsb_per_unit; the
    # last stage's own 2 rms(t_oracle - t64)), plus five standard deviations of a binomial count.
    g = SB.lsb_per_unit(cfg_name, inp, NB)
    budget = sum(g[st] * (SB.FACTOR_RMS * ref.err(st).rms + D[st][0]) for st in ("y", "v", "mpx")) + SB.FACTOR_RMS * SB.rms(t_o - ref.t64)
    n = ref.pcm.size
    diff = dev.pcm.astype(np.int32) - ref.pcm.astype(np.int32)
    share = float(np.mean(diff != 0))
    limit = budget + 5.0 * np.sqrt(budget * max(1.0 - budget, 0.0) / n)
    print("BUDGET %s flips share %.3e (limit %.3e: budget %.3e LSB, gains y %.3g v %.3g mpx %.3g LSB/unit), signed mean %+.3e LSB, max |diff| %d" %
          (label, share, limit, budget, g["y"], g["v"], g["mpx"], float(diff.mean()), int(np.abs(diff).max())))
    if share > limit:
        failures.append("pcm vs oracle, %s: %.3e of %d values differ, the stage budgets add up to %.3e (+ 5 sd = %.3e); signed mean %+.3e LSB" %
                        (label, share, n, budget, limit, float(diff.mean())))
    assert not failures, "\n".join(failures)
