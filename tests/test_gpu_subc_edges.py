"""The MPX subcarrier receiver on the device at the edges of the range fmdk_subc_check admits (csrc/subcarrier.inc), beside tests/test_gpu_subc.py,
whose helpers, bound and rules these tests use unchanged: every output within subc_model.subc_bound of the float64 model, bit equality across
the split into calls and the host form, exact zeros where the definition gives zero.  tests/test_subc_cpu.py shows on the CPU that the float32
model stays far inside the bound at every one of these shapes and that the planted defects still exceed it.

Shapes (subc_model.EDGE_SHAPES: rate, fc, bw, T, D, M) and the line of fmd_subc_kernel each is there for:
  (204800, 57050, 2400, 64, 8, 512)   Pd = 4096, the largest admitted: `bias` is Pd itself (Pd >= SC_H), and `p = p + 1 == Pd ? 0 : p + 1` never
                                      wraps within a chunk of SC_H + 512 staged samples - the index comes from `(p0 + 4 w) % Pd` alone
  (171000, 57000, 2400, 32, 4, 256)   Pd = 3: that wrap happens once or twice inside EVERY 4-sample word
  (228000, 57000, 2400, 16, 4, 4100)  Pd = 4 (a wrap per word); the block's second chunk is ns = D = 4 samples, no = 1: `oc[r] = o < no ? o : no - 1`
                                      sends 255 threads x 4 outputs each to output 0, and `if (o < no)` stores one
  (300000, 19000, 500, 256, 32, 4128) the same at D = 32, T = 256: that one output's history is the whole staged tail of chunk 0 (SC_H = T)
  (192000, 57000, 2400, 16, 4, 16)    M = T = 16, the smallest block: `nw = (SC_H + ns) >> 2` = 68 words, of which `rel + T >= 0` reads 8; `rel >= -T >= -M`
                                      reaches the whole block before it
  (300000, 57000, 2400, 32, 32, 32)   M = D = T: `no` = 1 in every workgroup of the launch, no history sample is ever used
  (300000, 19000, 500, 256, 4, 256)   `for (g = 0; g * D < T; g++)` runs 64 times, `col = SC_H / D - g` down to column 1; RO = 4 accumulators per thread
The last test is one launch whose v passes 2^32 bytes and whose sample index passes 2^29: `(size_t)sb * (size_t)M`, and `n0` in 32-bit unsigned
arithmetic."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subc_model as SM  # noqa: E402
from test_gpu_subc import R, assert_bound, input_of, make, run_dev, same_bits, taps_of  # noqa: E402,F401  (R: the module's fixture)

pytestmark = pytest.mark.gpu

S, NB = 3, 3


@pytest.mark.parametrize("shape", SM.EDGE_SHAPES)
def test_edge_shapes_match_the_model_and_do_not_depend_on_the_split(R, shape):
    """3 streams x 3 blocks from reset, LCG and tone input, every output within the bound; then the 3 blocks in one call = three single-block calls,
    the middle one through run_host, bit for bit"""
    rate, fc, bw, T, D, M = shape
    sub = make(R, shape, S)
    assert sub.out_per_block == M // D
    for kind in ("lcg", "tone"):
        v = input_of(kind, rate, fc, S, NB * M).reshape(S, NB, M)
        sub.reset()
        whole = run_dev(sub, v)
        assert_bound(whole, v, shape, "%s Pd %d T %d D %d M %d" % (kind, SM.period(rate, fc), T, D, M))
        if kind == "lcg":
            sub.reset()
            parts = np.concatenate([run_dev(sub, v[:, 0:1]), sub.run_host(v[:, 1:2], 1), run_dev(sub, v[:, 2:3])], axis=1)
            assert same_bits(parts, whole)
            for s in range(S):
                st = sub.get_state(s)
                assert st.phase == (NB * M) % SM.period(rate, fc)
                assert np.array_equal(np.array(st.hist[:T], dtype=np.float32).view(np.uint32), np.array(v[s].reshape(-1)[-T:]).view(np.uint32))
    sub.close()


@pytest.mark.parametrize("shape", SM.RAGGED_ONE_OUTPUT)
def test_an_impulse_on_chunk_0s_last_sample_reaches_the_one_output_of_the_ragged_chunk(R, shape):
    """v = a on sample 4095 of block 1 (sample count M + 4095), nothing else, 3 blocks: the output whose newest sample has the count n reads
    a c[(M + 4095) mod Pd] h[n - (M + 4095)].  The ragged chunk's single output (the block's last, n = 2 M - 1) is tap k = M - 4096; block 2's
    outputs go on through the taps and are exactly +0 past the filter's reach; block 0 is +0 throughout."""
    rate, fc, bw, T, D, M = shape
    amp = np.array([1.0, -2.5])
    at = M + 4095
    v = np.zeros((2, 3, M), dtype=np.float32)
    v[:, 1, 4095] = amp
    sub = make(R, shape, 2)
    got = run_dev(sub, v)
    sub.close()
    assert_bound(got, v, shape, "impulse before a one-output chunk, T %d D %d M %d" % (T, D, M))
    taps = taps_of(rate, bw, T).astype(np.float64)
    c = SM.carrier_exact(rate, fc, at, 1)[0]
    k = np.arange(3 * M // D) * D + D - 1 - at                          # the tap that meets the impulse, per output of the launch
    want = np.where((k >= 0) & (k < T), taps[np.clip(k, 0, T - 1)], 0.0)
    last = 2 * M // D - 1                                               # the ragged chunk's output
    assert k[last] == M - 4096 and want[last] != 0 and np.count_nonzero(want[last + 1:]) == (T - (M - 4096) - 1) // D
    for s in range(2):
        z = got[s].reshape(-1)
        assert np.abs(z.astype(np.complex128) - amp[s] * c * want).max() <= 4 * 2.0 ** -24 * 2 * abs(amp[s]) * np.abs(taps).max()
        assert z[last] != 0
        assert not z[want == 0].view(np.uint32).any()                   # before the impulse and past the filter's reach: exactly +0
        assert np.count_nonzero(z) == np.count_nonzero(want)


def test_a_launch_whose_v_passes_4_gib_and_whose_sample_index_passes_2_to_the_29(R):
    """(300000, 57000, 2400, 16, 32, 65536), 2 streams x 8193 blocks in ONE launch: v is 4.0 GiB (4.3e9 bytes), every block of stream 1 lies beyond 2 GiB and its
    last beyond 4 GiB; the sample index reaches 2^29 and Pd = 100 does not divide 2^32, so an index that wrapped or lost its top bits shows as a
    wrong carrier phase.  v is made on the device: zeros, an LCG burst across the common edge of stream 1's last two blocks, impulses on samples
    4096 and 4127 of stream 0's last block (16 taps at D = 32 read the upper half of each group of 32 alone: 4127 is tap 0 of chunk 1's first
    output, 4096 must not show) and a short LCG tail in both.  Only the blocks under test are downloaded: the last two of both streams are held
    to the bound from (phase ((nb - 2) M) mod Pd, zero history); the first and a middle block are exactly +0; the state after is the model's."""
    import torch
    shape = (300000, 57000, 2400, 16, 32, 65536)
    rate, fc, bw, T, D, M = shape
    n_s, nb, pd = 2, 8193, SM.period(rate, fc)
    assert pd == 100 and n_s * nb * M * 4 > 2 ** 32 and nb * M > 2 ** 29 and ((nb - 2) * M) % pd != 0
    dev = torch.device("cuda:0")
    sub = make(R, shape, n_s)
    d_v = torch.zeros((n_s, nb, M), dtype=torch.float32, device=dev)
    d_z = torch.full((n_s, nb, M // D, 2), -7.0, dtype=torch.float32, device=dev)
    burst, tails = SM.lcg_floats(96, 3), [SM.lcg_floats(24, 5), SM.lcg_floats(24, 6)]
    d_v[1, nb - 2, M - 48:] = torch.from_numpy(burst[:48]).to(dev)
    d_v[1, nb - 1, :48] = torch.from_numpy(burst[48:]).to(dev)
    d_v[0, nb - 1, 4096] = 1.5
    d_v[0, nb - 1, 4127] = -0.75
    for s in range(n_s):
        d_v[s, nb - 1, M - 24:] = torch.from_numpy(tails[s]).to(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub.run_device(d_v, nb, d_z)
    sub.sync()
    print("2 x %d blocks of %d samples (v %.2f GiB): %.3f s from launch to sync" % (nb, M, n_s * nb * M * 4 / 2.0 ** 30, time.perf_counter() - t0))
    v_end = d_v[:, nb - 2:].cpu().numpy()
    z_end = d_z[:, nb - 2:].cpu().numpy().view(np.complex64)[..., 0]
    assert np.count_nonzero(v_end[0]) == 2 + 24 and np.count_nonzero(v_end[1]) >= 96 + 24 - 4
    assert_bound(z_end, v_end, shape, "past 4 GiB", hist=np.zeros((n_s, T), dtype=np.float32), phase=((nb - 2) * M) % pd)
    assert z_end[0, 1, 4096 // D] != 0 and np.count_nonzero(z_end[0]) == 2 and np.count_nonzero(z_end[1]) == 4     # (one output per 16 samples read)
    for b in (0, nb // 2):
        assert not d_z[:, b].cpu().numpy().view(np.uint32).any(), b     # written, and exactly +0
    for s in range(n_s):
        st = sub.get_state(s)
        assert st.phase == (nb * M) % pd
        assert np.array_equal(np.array(st.hist[:T], dtype=np.float32).view(np.uint32), tails[s][-T:].view(np.uint32))
    sub.close()
