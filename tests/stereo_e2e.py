"""What tests/test_stereo_cpu.py and tests/test_gpu_stereo.py share about the end-to-end case: the DDS multiplex of the oracle with and without
its pilot through the float64 chain (tests/chain_f64.py) and the float64 subcarrier model at 19 kHz, block by block, and the thresholds the GPU test
takes from the two: pilot_on^2 = twice their geometric mean, pilot_off^2 = half of it."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_f64 as C64  # noqa: E402
import subc_model as SM  # noqa: E402

PILOT_SIZES = (1, 255, 256, 257, 4096)                  # Mz of the pilot meter's own GPU test
# block_len: the chain's start (zero decimator history, no sample before the first) is one wide-band click in v; through the 128-tap filter it fills
# 8 outputs of block 0 with |z| up to 0.05.  At 16384 bytes (64 outputs a block) that is a pilot_ms of 4.0e-4 without any pilot, a factor of 56
# below the pilot's; at 65536 (256 outputs) the same click is a quarter of that.  The factor of 100 is asked of every block, the first included.
RATE, BLOCK_LEN, N_BLOCKS = 300000, 65536, 5
FC, BW, N_TAPS, DECIM = 19000, 500, 128, 16             # the defaults of BatchDemod.subcarrier
HOLD = 2


@functools.lru_cache(maxsize=None)
def dds_iq(stereo):
    from oracle import dds_bytes
    iq = dds_bytes(BLOCK_LEN * N_BLOCKS, stereo=stereo)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def pilot_ms_f64_of_dds(stereo):
    """float64 [N_BLOCKS]: mean |z|^2 per block of the 19 kHz receiver over the float64 discriminator output"""
    import rtl_fm_player_amd as R
    fb = np.array(R.design_taps(R.wbfm_config(rate_in=RATE, block_len=BLOCK_LEN)).fb[:], dtype=np.float32)
    y = C64.decimate(dds_iq(stereo), None, 0, fb)
    v = C64.discriminate(y)
    z, _ = SM.subc_f64(v, SM.design(RATE, BW, N_TAPS).astype(np.float32), RATE, FC, DECIM)
    mz = BLOCK_LEN // 16 // DECIM
    return (np.abs(np.asarray(z).reshape(N_BLOCKS, mz)) ** 2).mean(axis=1)


def thresholds():
    """(pilot_on, pilot_off) as floats"""
    gm = float(np.sqrt(pilot_ms_f64_of_dds(1).min() * pilot_ms_f64_of_dds(0).max()))
    return float(np.sqrt(2.0 * gm)), float(np.sqrt(0.5 * gm))
