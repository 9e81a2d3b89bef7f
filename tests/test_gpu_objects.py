"""What the receiver objects share (csrc/fmd_dev.c: the core fmd_subc, fmd_tuner, fmd_scan and fmd_rds embed), on the device: state access per
element, staging that grows and is reused smaller, and close with work still queued on a caller's stream.  Each object's own test module holds it to
its model; here only what one implementation now serves for all of them, at each object's smallest shape (the first of its module's), three streams
or sources, at most five blocks in all.  The scan carries no state and its result belongs to a launch, not to a block: it takes part where that
applies."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_model as M  # noqa: E402
import test_gpu_rds as TR  # noqa: E402
import test_gpu_scan as TC  # noqa: E402
import test_gpu_subc as TS  # noqa: E402
import test_gpu_tuner as TT  # noqa: E402
import tuner_model as TM  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3                                                   # streams (tuner: sources, one channel each)
SUBC, RDS, TUNER, SCAN = TS.SHAPES[0], TR.SHAPES[0], TM.MODEL_CASES[0], M.CASES[0]
RDS_KEYS = ("soft", "lens", "first", "est")


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


def make(R, kind):
    if kind == "subc":
        return TS.make(R, SUBC, N)
    if kind == "rds":
        return TR.make(R, RDS, N)
    if kind == "tuner":
        _, _, T, P, shift, gain, bl, _ = TUNER
        return TT.make(R, T, P, bl, N, [(s, shift, gain) for s in range(N)])
    return R.Scan(TC.c_config(R, SCAN[1]), N)


def blocks(kind, nb):
    """nb blocks of input per stream, [N, nb, ...], every stream its own values"""
    if kind == "subc":
        rate, fc, _, _, _, m = SUBC
        return TS.input_of("lcg", rate, fc, N, nb * m).reshape(N, nb, m)
    if kind == "rds":
        return TR.input_of("lcg", RDS[0], N, nb * RDS[2]).reshape(N, nb, RDS[2])
    if kind == "tuner":
        return TT.sources(TUNER[1], TUNER[6], nb, n_src=N)
    return M.case_power(SCAN[4], SCAN[1], nb, N)


def run_dev(kind, obj, x):
    """one run_device call, waited for: the module's own helper (the tuner's bytes without its y)"""
    if kind == "tuner":
        return TT.run_dev(obj, x, want_y=False)[0]
    return {"subc": TS.run_dev, "rds": TR.run_dev, "scan": TC.run_dev}[kind](obj, x)


def run_host(kind, obj, x):
    """one run_host call, in the form run_dev returns"""
    out = obj.run_host(x, x.shape[1])
    if kind == "rds":
        return dict(zip(RDS_KEYS, out))
    if kind == "scan":
        return out[0].view(M.STATION_DTYPE), out[1], out[2]
    return out


def same_bits(kind, a, b):
    return {"subc": TS.same_bits, "rds": TR.same_bits, "tuner": lambda p, q: p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes(),
            "scan": TC.same_bits}[kind](a, b)


def cat(kind, parts):
    return TR.cat(parts) if kind == "rds" else np.concatenate(parts, axis=1)


def modified(kind, st):
    """a valid copy of a state that differs from it: inside every range fmd_*_set_state checks"""
    x = type(st).from_buffer_copy(bytes(st))
    if kind == "subc":
        x.hist[0] += 1.5
    elif kind == "tuner":
        x.hist[0] ^= 0x55
    else:
        x.bit += 1
        x.zhist[0] += 0.25
    return x


@pytest.mark.parametrize("kind", ["subc", "tuner", "rds"])
def test_state_access_is_per_element(R, kind):
    obj = make(R, kind)
    run_dev(kind, obj, blocks(kind, 1))
    before = [bytes(obj.get_state(i)) for i in range(N)]
    assert all(any(b) for b in before) and len(set(before)) == N            # one block in: non-zero, and every element its own
    x = modified(kind, obj.get_state(1))
    obj.set_state(1, x)
    assert bytes(obj.get_state(1)) == bytes(x) != before[1]
    assert bytes(obj.get_state(0)) == before[0] and bytes(obj.get_state(2)) == before[2]
    for bad in (-1, N):
        with pytest.raises(R.FmdError, match=r"failed \(-1\)"):             # FMD_E_ARG
            obj.get_state(bad)
        with pytest.raises(R.FmdError, match=r"failed \(-1\)"):
            obj.set_state(bad, x)
    assert bytes(obj.get_state(1)) == bytes(x) and bytes(obj.get_state(0)) == before[0] and bytes(obj.get_state(2)) == before[2]
    obj.reset()
    for i in range(N):
        assert not any(bytes(obj.get_state(i))), i
    obj.close()


@pytest.mark.parametrize("kind", ["subc", "tuner", "rds", "scan"])
def test_the_staging_grows_and_is_reused_smaller(R, kind):
    """run_host with 1, then 3, then 1 blocks of consecutive input on one object against run_device on a fresh one: the five blocks in one launch -
    the scan, whose result is a launch's, call by call"""
    five = blocks(kind, 5)
    obj, fresh = make(R, kind), make(R, kind)
    parts = [run_host(kind, obj, five[:, a:b]) for a, b in ((0, 1), (1, 4), (4, 5))]
    if kind == "scan":
        for part, (a, b) in zip(parts, ((0, 1), (1, 4), (4, 5))):
            assert same_bits(kind, part, run_dev(kind, fresh, five[:, a:b])), (a, b)
    else:
        assert same_bits(kind, cat(kind, parts), run_dev(kind, fresh, five))
    obj.close()
    fresh.close()


def launch(kind, obj, x, stream):
    """queue one run_device of x on a torch stream and return the output tensors without waiting"""
    import torch
    dev = torch.device("cuda:0")
    nb = x.shape[1]
    d_in = torch.from_numpy(np.ascontiguousarray(x).view(np.float32 if kind == "rds" else x.dtype).reshape(-1).copy()).to(dev)
    if kind == "subc":
        outs = [torch.full((N, nb, obj.out_per_block, 2), -7.0, dtype=torch.float32, device=dev)]
    elif kind == "tuner":
        outs = [torch.full((N, nb, x.shape[2]), 77, dtype=torch.uint8, device=dev), None]
    elif kind == "rds":
        outs = [torch.full((N, nb, obj.bits_per_block), -7.0, dtype=torch.float32, device=dev), torch.full((N, nb), -7, dtype=torch.int32, device=dev),
                torch.full((N, nb), -7, dtype=torch.int64, device=dev), torch.full((N, nb, 4), -7.0, dtype=torch.float32, device=dev)]
    else:
        outs = [torch.full((N, obj.cfg.max_stations * 32), 255, dtype=torch.uint8, device=dev), torch.full((N, 2), -1, dtype=torch.int32, device=dev),
                torch.full((N, obj.n_candidates), -7.0, dtype=torch.float32, device=dev)]
    torch.cuda.synchronize()                            # the buffers are ready before the other stream reads them
    obj.run_device(d_in, nb, *outs, hip_stream=stream.cuda_stream)
    return [o for o in outs if o is not None], d_in


@pytest.mark.parametrize("kind", ["subc", "tuner", "rds", "scan"])
def test_close_waits_for_work_queued_on_a_callers_stream(R, kind):
    """close() right behind a launch on a caller's stream: the launch still reads the object's tables and state, so close has to wait for that
    stream - the output equals that of the same launch on a second object that was synced before it was closed"""
    import torch
    x = blocks(kind, 3)
    a, b = make(R, kind), make(R, kind)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got, keep_a = launch(kind, a, x, sa)
    a.close()
    torch.cuda.synchronize()
    want, keep_b = launch(kind, b, x, sb)
    b.sync()
    b.close()
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    del keep_a, keep_b
