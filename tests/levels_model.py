"""Python models of the batch API's channel level and power squelch (include/fmdemod_mi355x.h, "Channel level and power squelch"),
for tests/test_levels_cpu.py and tests/test_gpu_levels.py."""
import numpy as np


def block_level(y):
    """The reference's rms() (src/rtl_fm_player.c:737-755, step = 1) over one block's lowpassed buffer y (2 M interleaved I/Q floats), in
    float64 and without its integer truncation: sqrt(max(0, S2/n - (S1/n)^2))."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    s1, s2 = y.sum(), (y * y).sum()
    return float(np.sqrt(max(0.0, s2 / n - (s1 / n) ** 2))), s2 / n


def squelch_model(levels, thresholds, conseq, hits0=None):
    """rtl_fm's power squelch over levels [n_streams, n_blocks] (float32, as the library returns them): (closed [S, B] bool, final hits [S]).
    thresholds[s] <= 0: off for that stream (never closed, hits untouched).  hits0: the counters before the first block (default conseq + 1)."""
    levels = np.asarray(levels, dtype=np.float32)
    S, B = levels.shape
    hits = [conseq + 1] * S if hits0 is None else list(hits0)
    closed = np.zeros((S, B), dtype=bool)
    for s in range(S):
        t = np.float32(thresholds[s])
        if not t > 0:
            continue
        h = hits[s]
        for b in range(B):
            h = h + 1 if levels[s, b] < t else 0
            if h > conseq:
                h = conseq + 1
                closed[s, b] = True
        hits[s] = h
    return closed, hits
