"""The RDS receiver on the device at the edges of the range fmdk_rds_check admits (csrc/rds.inc), beside tests/test_gpu_rds.py,
whose helpers, bounds and rules these tests use unchanged: y, Tm, sum p, Ts and the soft bits within rds_model's bounds of the float64 model,
integers equal, phi by DESIGN.md section 2b's rule, bit equality across the split into calls, the host form and a captured graph.
tests/test_rds_cpu.py shows on the CPU that the float32 model stays inside the bounds at every one of these shapes, that the planted defects
exceed them, that a zero left in a bit past the 256th or a dropped chunk partial cannot pass, and that the synthesised input leaves the phi rule
its six blocks.

Shapes (rds_model.EDGE_SHAPES: (rate_z, Tg, Bz), blocks, streams) and the lines of csrc/rds.inc each is there for:
  (38000, 64, 68) x 12      S = 32, Hy = 66 > RD_H = 64: the state kernel's `if (t < g.hy)` copies 66 values and the slicer's `st->yhist[idx + d]` reads
                            them; a block lies almost wholly in its own lookback (`rel >= -Hy >= -Bz`), 2 or 3 bits in a slot of 4; Pw = 32
  (37875, 64, 128) x 12     Pw = 606 of FMD_RDS_MAX_PERIOD = 640: `w[(p0 + o) % Pw]`, p0 = 128 b mod 606; S = 31.89
  (37875, 16, 68) x 12      `gt[t] = t < Tg ? taps[t] : 0` with 48 zeros, `rel + Tg >= 0` reads 16 of the 64 staged samples, beside the longest lookback
  (11875, 16, 2816) x 3     S = 10 exactly, Pw = 10; 281 / 282 bits in a slot of 284: the slicer's `for (j = t; j < g.slot; j += RD_NT)` goes round twice;
                            cpb = 3, the last chunk ragged (`ns` = 768): the tracker's `for (c = 0; c < cpb; c++)` past 2
  (12000, 32, 4096) x 3     405 / 406 bits in a slot of 408, 4 whole chunks
  (18750, 64, 65536) x 2    one stream; cpb = 64, 4150 / 4151 bits: 17 trips of the slicer's loop, the `chunks` term of tm_bound at its largest
  (38000, 64, 65536) x 2    one stream; count 2048 = slot: `j < count` holds for every j, nothing is zeroed
At Bz = 65536 the phi rule would need more blocks than a few seconds allow: there phi is held through the integers and through the soft bits
sliced with the device's own phi, as hold_to_the_model does everywhere.
The LCG input's stream 0 is seed 77, the input of the CPU teeth.  The last test is one launch whose z and y pass 2^32 bytes: `(size_t)sb * (size_t)Bz`,
and `p0` in 32-bit unsigned arithmetic past 2^28."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rds_model as RM  # noqa: E402
from test_gpu_rds import AVG, R, cat, hold_to_the_model, make, run_dev, same_bits, taps_of  # noqa: E402,F401  (R: the module's fixture)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def input_of(kind, shape, S, nb):
    """complex64 [S, nb, Bz], read-only; every stream its own values"""
    rate_z, _, Bz = shape
    n = nb * Bz
    if kind == "lcg":
        a = np.stack([RM.lcg_complex(n, 77 + 13 * s) for s in range(S)])
    elif kind == "zeros":
        a = np.zeros((S, n), dtype=np.complex64)
    elif kind == "rds":
        a = RM.synth_z(rate_z, S, n, max(4, RM.groups_to_fill(rate_z, n)))
    else:
        raise ValueError(kind)
    a = a.reshape(S, nb, Bz)
    a.setflags(write=False)
    return a


def states_of(rds, S):
    return [bytes(rds.get_state(s)) for s in range(S)]


@pytest.mark.parametrize("shape,nb,S", RM.EDGE_SHAPES)
def test_edge_shapes_match_the_model(R, shape, nb, S):
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    rds = make(R, shape, S, max_blocks=nb)
    assert rds.bits_per_block == geo.slot
    for kind in ("lcg", "zeros", "rds"):
        z = input_of(kind, shape, S, nb)
        rds.reset()
        got = run_dev(rds, z)
        y_dev, tm_dev = rds.last_y(nb)
        e_dev, e_ref, mag = [], [], []
        for s in range(S):
            a, b, c = hold_to_the_model({k: v[s] for k, v in got.items()}, y_dev[s], tm_dev[s], z[s], shape, "%s %s stream %d" % (kind, shape, s))
            e_dev.append(a); e_ref.append(b); mag.append(c / max(c.max(), 1e-300))
        if kind == "zeros":
            assert not got["soft"].view(np.uint32).any() and not got["est"][..., :2].any() and not y_dev.view(np.uint32).any()
        if kind == "lcg" and geo.slot == 2048:
            assert (got["lens"] == geo.slot).all() and np.count_nonzero(got["soft"]) >= got["soft"].size - 4      # a full slot: every bit is data
        if kind == "rds" and Bz < 65536:
            e_dev, e_ref, mag = np.concatenate(e_dev), np.concatenate(e_ref), np.concatenate(mag)
            keep = mag > 0.25
            rms = lambda x: float(np.sqrt(np.mean(x * x)))  # noqa: E731
            print("phi %s: %d blocks, device rms %.3g worst %.3g; float32 model rms %.3g worst %.3g" %
                  (shape, keep.sum(), rms(e_dev[keep]), np.abs(e_dev[keep]).max(), rms(e_ref[keep]), np.abs(e_ref[keep]).max()))
            assert keep.sum() >= 6
            assert rms(e_dev[keep]) <= 2 * rms(e_ref[keep])
            assert np.abs(e_dev[keep]).max() <= 3 * np.abs(e_ref[keep]).max()
    rds.close()


@pytest.mark.parametrize("shape,nb,S", RM.EDGE_SHAPES)
def test_split_invariance_at_the_edge_shapes(R, shape, nb, S):
    """all blocks in one call = 1 + the rest = single blocks = the host form, bit for bit, and the state after is the same bytes; with single
    blocks every block's first pair comes from the carried y history (Hy = 66 values at S = 32)"""
    z = input_of("rds", shape, S, nb)
    rds = make(R, shape, S, max_blocks=nb)
    whole = run_dev(rds, z)
    states = states_of(rds, S)
    assert whole["lens"].min() >= 0 and whole["soft"].any()
    rds.reset()
    assert same_bits(cat([run_dev(rds, z[:, :1]), run_dev(rds, z[:, 1:])]), whole)
    assert states_of(rds, S) == states
    rds.reset()
    assert same_bits(cat([run_dev(rds, z[:, k:k + 1]) for k in range(nb)]), whole)
    assert states_of(rds, S) == states
    rds.reset()
    k = max(nb - 2, 1)
    host = cat([dict(zip(("soft", "lens", "first", "est"), rds.run_host(z[:, :k], k))), dict(zip(("soft", "lens", "first", "est"), rds.run_host(z[:, k:], nb - k)))])
    assert same_bits(host, whole)
    assert states_of(rds, S) == states
    rds.close()


@pytest.mark.parametrize("shape,nb,S", RM.EDGE_SHAPES)
def test_state_hand_over_at_the_edge_shapes(R, shape, nb, S):
    """get_state after k blocks is the model's integers, the last Tg z, the last Hy y of the launch (bit for bit) and the last block's Ts;
    set_state into a fresh object, streams crossed over, continues bit-equal"""
    rate_z, Tg, Bz = shape
    geo = RM.Geometry(rate_z, Bz)
    k = nb // 2
    z = input_of("rds", shape, S, nb)
    rds = make(R, shape, S, max_blocks=nb)
    whole = run_dev(rds, z)
    rds.reset()
    first = run_dev(rds, z[:, :k])
    y_dev, _ = rds.last_y(k)
    states = [rds.get_state(s) for s in range(S)]
    for s in range(S):
        _, st = RM.receive(z[s, :k].reshape(-1), geo, taps_of(rate_z, Tg), AVG)
        assert (states[s].phase, states[s].frac + RM.Q * geo.lb, states[s].bit) == (st.phase, st.e, st.bit) and st.phase == (k * Bz) % geo.pw
        assert np.array_equal(np.array(states[s].zhist[:2 * Tg], dtype=np.float32).view(np.complex64), z[s, k - 1, Bz - Tg:])
        assert np.array(states[s].yhist[:2 * geo.hy], dtype=np.float32).tobytes() == y_dev[s, k - 1, Bz - geo.hy:].tobytes() and y_dev[s, k - 1, Bz - 2:].all()
        assert (states[s].ts[0], states[s].ts[1]) == (first["est"][s, k - 1, 0], first["est"][s, k - 1, 1])
    fresh = make(R, shape, S, max_blocks=nb)
    for s in range(S):
        fresh.set_state(s, states[S - 1 - s])
    rest = run_dev(fresh, z[::-1, k:])
    assert same_bits(cat([first, {k_: v[::-1] for k_, v in rest.items()}]), whole)
    fresh.close()
    rds.close()


def test_a_captured_graph_of_a_multi_chunk_launch_replays_to_the_bits_of_the_eager_launch(R):
    """(11875, 16, 2816): the four kernels of a 2-block launch (3 chunks per block, 281 / 282 bits) captured once on one torch stream, no branches,
    and replayed three times with z refilled in between: bit-equal to eager launches, and the state after is the same bytes"""
    import torch
    shape = (11875, 16, 2816)
    rate_z, Tg, Bz = shape
    S, nb, reps = 3, 2, 3
    z = input_of("rds", shape, S, reps * nb).reshape(S, reps, nb, Bz)
    dev = torch.device("cuda:0")
    eager, graphed = make(R, shape, S, max_blocks=nb), make(R, shape, S, max_blocks=nb)
    want = [run_dev(eager, z[:, r]) for r in range(reps)]
    d_z = torch.zeros((S, nb, Bz, 2), dtype=torch.float32, device=dev)
    d_soft = torch.zeros((S, nb, graphed.bits_per_block), dtype=torch.float32, device=dev)
    d_lens = torch.zeros((S, nb), dtype=torch.int32, device=dev)
    d_first = torch.zeros((S, nb), dtype=torch.int64, device=dev)
    d_est = torch.zeros((S, nb, 4), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream()
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
        assert got["lens"].min() > 256
    assert states_of(graphed, S) == states_of(eager, S)
    eager.close()
    graphed.close()


def test_a_launch_whose_z_and_y_pass_4_gib(R):
    """(18750, 64, 65536), 2 streams x 4100 blocks in ONE launch (max_blocks = 4100): z and the y scratch are 4.0 GiB (4.3e9 bytes) each, every block of stream 1
    lies beyond 2 GiB and its last beyond 4 GiB; the table index passes 2^28 and Pw = 300 does not divide 2^32, so an index that wrapped or
    lost its top bits shows in Tm.  z is made on the device: zeros, and an LCG burst over the common edge of stream 1's last two blocks.  The model
    runs from the state 4098 zero blocks leave (the sample count mod Pw, the next bit and its offset from rds_model.block_counts, Ts = 0, zero
    histories).  The last two blocks of both streams: counts and first-bit indices (about 1.7e7) equal, y, Tm, sum p, Ts and the soft bits
    within their bounds; the state after is the model's integers; the first block's outputs are +0."""
    import torch
    shape = (18750, 64, 65536)
    rate_z, Tg, Bz = shape
    S, nb, half = 2, 4100, 3072
    geo = RM.Geometry(rate_z, Bz)
    assert S * nb * Bz * 8 > 2 ** 32 and (nb - 1) * Bz > 2 ** 28 and geo.pw == 300
    dev = torch.device("cuda:0")
    rds = make(R, shape, S, max_blocks=nb)
    d_z = torch.zeros((S, nb, Bz, 2), dtype=torch.float32, device=dev)
    burst = RM.lcg_complex(2 * half, 5)
    d_z[1, nb - 2, Bz - half:] = torch.from_numpy(burst[:half].view(np.float32).reshape(half, 2).copy()).to(dev)
    d_z[1, nb - 1, :half] = torch.from_numpy(burst[half:].view(np.float32).reshape(half, 2).copy()).to(dev)
    d_soft = torch.full((S, nb, geo.slot), -7.0, dtype=torch.float32, device=dev)
    d_lens = torch.full((S, nb), -7, dtype=torch.int32, device=dev)
    d_first = torch.full((S, nb), -7, dtype=torch.int64, device=dev)
    d_est = torch.full((S, nb, 4), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rds.run_device(d_z, nb, d_soft, d_lens, d_first, d_est)
    rds.sync()
    print("2 x %d blocks of %d samples (z %.2f GiB): %.3f s from launch to sync" % (nb, Bz, S * nb * Bz * 8 / 2.0 ** 30, time.perf_counter() - t0))
    z_end = d_z[:, nb - 2:].cpu().numpy().view(np.complex64)[..., 0]
    got = dict(soft=d_soft[:, nb - 2:].cpu().numpy(), lens=d_lens[:, nb - 2:].cpu().numpy(), first=d_first[:, nb - 2:].cpu().numpy(),
               est=d_est[:, nb - 2:].cpu().numpy())
    y_all, tm_all = rds.last_y(nb)                       # (the API hands out the whole launch's y; the two blocks under test are kept)
    y_end, tm_end = y_all[:, nb - 2:].copy(), tm_all[:, nb - 2:].copy()
    assert not tm_all[:, :nb - 2].view(np.uint32).any()
    del y_all
    _, counts, e = RM.block_counts(geo, RM.Q * geo.lb, nb - 2)
    start = RM.State(geo, Tg)
    start.phase, start.e, start.bit = ((nb - 2) * Bz) % geo.pw, e, int(np.sum(counts))
    assert start.phase != 0 and start.bit > 1.7e7
    for s in range(S):
        hold_to_the_model({k: v[s] for k, v in got.items()}, y_end[s], tm_end[s], z_end[s], shape, "past 4 GiB, stream %d" % s, state=start)
        _, after = RM.receive(z_end[s].reshape(-1), geo, taps_of(rate_z, Tg), AVG, state=start)
        st = rds.get_state(s)
        assert (st.phase, st.frac + RM.Q * geo.lb, st.bit) == (after.phase, after.e, after.bit) and after.phase == (nb * Bz) % geo.pw
    assert np.count_nonzero(got["soft"][1]) > 2 * half // 16 - 16 and abs(tm_end[1, 0]) > 0 and not got["soft"][0].view(np.uint32).any()
    est0 = d_est[:, 0].cpu().numpy()
    assert not d_soft[:, 0].cpu().numpy().view(np.uint32).any() and not est0[:, [0, 1, 3]].view(np.uint32).any() and (est0[:, 2] == 0).all()      # (phi of Ts = 0 is -0)
    assert (d_lens[:, 0].cpu().numpy() == counts[0]).all() and not d_first[:, 0].cpu().numpy().any()
    rds.close()
