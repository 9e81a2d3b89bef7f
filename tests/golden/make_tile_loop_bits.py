#!/usr/bin/env python3
"""Generate tests/golden/tile_loop_bits.json: PCM + lens hashes of the fast kernel families on an MI355X.

    FMD_LIB_PATH=<library of the commit to record> python tests/golden/make_tile_loop_bits.py <commit id>       (needs a gfx950 device)

The +-1 LSB families are free to differ from the oracle in the last bit, so their exact bits are pinned by what a NAMED BUILD computed on
gfx950: a change that claims to leave the arithmetic alone (an instruction removed, a constant read from somewhere else) must reproduce them
bit for bit - tests/test_gpu_tile_loop_bits.py.  Inputs every machine regenerates (oracle.lcg_bytes, oracle.dds_bytes); per case TWO consecutive
launches of `blocks` blocks each, so that the carried state of the first is what the second starts from.  The hash is oracle.hash16 over the
valid PCM of all streams, blocks and both launches in order, continued over the block lengths (int32, as int16 pairs).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BL = 262144
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_loop_bits.json")
# the configurations of tests/test_gpu_parity.py CONFIGS (every flush form: stereo_300k runs flush_g 3)
CONFIGS = {
    "stereo_300k": dict(rate_in=300000, rate_out2=48000, mode=2),
    "mono_300k": dict(rate_in=300000, rate_out2=48000, mode=1),
    "nfm_25k": dict(rate_in=25000, rate_out2=12500, mode=1),
    "stereo_240k": dict(rate_in=240000, rate_out2=48000, mode=2),
    "stereo_192k": dict(rate_in=192000, rate_out2=48000, mode=2),
}
# (streams, blocks per launch): one chunk per stream; chunks that start in mid-block; block ends inside a chunk
SHAPES = [(1, 2), (3, 4), (8, 8)]
FAMILIES = ["FAST", "FAST_MFMA_F"]
INPUTS = ["lcg", "fm"]


def case_id(name, shape, family, kind):
    return "%s-%dx%d-%s-%s" % (name, shape[0], shape[1], family, kind)


_cache = {}


def make_input(kind, streams, blocks):
    """uint8 [streams][2 * blocks][BL]: LCG noise per stream (seed 7000 + s); kind 'fm': stream 0 is the integer-DDS stereo broadcast instead."""
    from oracle import dds_bytes, lcg_bytes
    key = (kind, streams, blocks)
    if key not in _cache:
        n = 2 * blocks * BL
        rows = [lcg_bytes(n, 7000 + s)[0] for s in range(streams)]
        if kind == "fm":
            rows[0] = dds_bytes(n)
        _cache[key] = np.stack(rows).reshape(streams, 2 * blocks, BL)
        _cache[key].setflags(write=False)
    return _cache[key]


def run_case(R, name, shape, family, kind):
    """The case's hash with the library R has loaded."""
    from oracle import hash16
    streams, blocks = shape
    iq = make_input(kind, streams, blocks)
    b = R.BatchDemod(R.wbfm_config(block_len=BL, math=getattr(R, "MATH_" + family), **CONFIGS[name]), streams)
    pcm, lens = [], []
    for launch in range(2):
        out, ln = b.run_host_concat(np.ascontiguousarray(iq[:, launch * blocks:(launch + 1) * blocks]), blocks)
        pcm += [out[s] for s in range(streams)]
        lens.append(np.asarray(ln, dtype=np.int32))
    b.close()
    h = hash16(np.concatenate(pcm))
    return hash16(np.concatenate([x.reshape(-1) for x in lens]).view(np.int16), h)


def main(commit):
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    hashes = {}
    for name in sorted(CONFIGS):
        for shape in SHAPES:
            for family in FAMILIES:
                for kind in INPUTS:
                    hashes[case_id(name, shape, family, kind)] = "%016x" % run_case(R, name, shape, family, kind)
    doc = {"what": "oracle.hash16 over PCM then lens of two consecutive launches; results of the named commit's build on gfx950 (MI355X)",
           "commit": commit, "hashes": hashes}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (OUT, len(hashes)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "unknown")
