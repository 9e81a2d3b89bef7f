"""The fast kernel families compute the same BITS as the build whose results are recorded in tests/golden/tile_loop_bits.json.

Against the oracle the +-1 LSB families may move by a last bit; a change of the tile loop that touches no arithmetic (a launch constant read
from a register instead of the kernarg segment, a lane map made once instead of per tile) may not: PCM and block lengths of two consecutive
launches - the second starts from the state the first handed over - hash to what that build produced on the same inputs.  The hashes are
gfx950 (MI355X) results of the commit named in the file (tests/golden/make_tile_loop_bits.py regenerates them from a library of choice).
A mismatch is a failure: there is no +-1 LSB here.

Configurations: those of test_gpu_parity.CONFIGS (every flush form: stereo_300k is flush_g 3, stereo_240k / _192k 4, mono_300k 2, nfm_25k 4 with
the wide second stage); shapes (streams, blocks per launch) (1, 2), (3, 4), (8, 8) at block_len 262144: one chunk per stream, chunks that start
in mid-block, block ends inside a chunk; inputs: LCG noise (the cold paths run) and an FM-like stream (the integer-DDS stereo broadcast).
"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_tile_loop_bits as G  # noqa: E402


@pytest.fixture(scope="module")
def R():
    import rtl_fm_player_amd as R
    if R.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need a real MI355X")
    return R


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        doc = json.load(f)
    assert len(doc["commit"]) >= 7 and len(doc["hashes"]) == len(G.CONFIGS) * len(G.SHAPES) * len(G.FAMILIES) * len(G.INPUTS)
    return doc["hashes"]


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("shape", G.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(G.CONFIGS))
def test_two_launches_hash_to_the_recorded_bits(R, golden, name, shape, family):
    for kind in G.INPUTS:
        got = "%016x" % G.run_case(R, name, shape, family, kind)
        assert got == golden[G.case_id(name, shape, family, kind)], "%s: PCM / lens bits differ from the recorded build's" % G.case_id(name, shape, family, kind)
