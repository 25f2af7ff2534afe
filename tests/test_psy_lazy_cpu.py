"""Short-block psychoacoustics only where they are read, CPU tier (tests/psy_lazy_cases.py): every case through the one-lane and through the
64-lane simulation with LAMEJS_PSY_LAZY_MIN_FRAMES=0 (every batch on the separate kernels lazy) against the same library with the hook at
"never" and against the oracle -- MP3 bytes, the stream state after every call, and lhip_debug_read(2) against lhip_debug_read(1): every long
entry bit for bit, the short entries bit for bit where needS holds by definition and all zero elsewhere.  The counts of needS / needF are those
of the parent's host simulation on the same material; stereo `bursts` must show at least 40 calls zeroed and 8 computed, `sine` at least 70
zeroed, and no eager short block is all zero, so a zero can only be a skip."""
import pytest

import psy_lazy_cases as pl
from libs import sim_library

KINDS = ("hostsim", "wavesim")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c["name"] for c in pl.CASES])
def test_psy_lazy_case(kind, name):
    lib = sim_library(kind)
    counts, _ = pl.check_case(lib, name)
    assert len(counts) == 1
    zeroed, computed, needS, needF = counts[0]
    print(kind, name, "zeroed", zeroed, "computed", computed, "needS", needS, "needF", needF)
    expect = pl.case(name)["expect"]
    if expect is not None:
        assert (zeroed + computed, needS, needF) == expect, (name, zeroed, computed, needS, needF)
    assert computed == needS and zeroed > 0 and computed > 0
    if name == "stereo128/bursts":
        assert zeroed >= 40 and computed >= 8, (zeroed, computed)
    if name == "stereo128/sine":
        assert zeroed >= 70, zeroed


@pytest.mark.parametrize("kind", KINDS)
def test_psy_lazy_three_streams_in_one_batch(kind):
    zeroed, computed = pl.check_three_streams(sim_library(kind))
    print(kind, "three streams: zeroed", zeroed, "computed", computed)
    assert zeroed > 0 and computed >= 3


@pytest.mark.parametrize("kind", KINDS)
def test_psy_lazy_calls_cut_around_the_first_short_granule(kind):
    """One `bursts` stream in six calls, cut at every granule boundary from two granules before its first short granule to two after: the granule that
    reads a call's short thresholds lies in the next batch (the last call of a batch always keeps its short side), and the batches of one granule
    between the two large ones take the one-frame program."""
    lib = sim_library(kind)
    name = "stereo128/bursts"
    L, R, _ = pl.material(name)
    whole = pl.encode_calls(sim_library("hostsim"), pl.case(name), L, R, [len(L)], pl.NEVER)      # (where the first short block lies: the quick simulation)
    g = pl.first_short_granule(whole["calls"][0]["bt"])
    assert g >= 3, g
    cuts = [576 * (g + d) for d in (-2, -1, 0, 1, 2)]
    lens = [cuts[0], 576, 576, 576, 576, len(L) - cuts[-1]]
    counts, cut = pl.check_case(lib, name, lens)
    print(kind, "first short granule", g, "calls", [(c["frames"], sorted(c["paths"])) for c in cut["calls"]], "counts", counts)
    assert len(counts) == 2 and all(z > 0 and n > 0 for z, n, _, _ in counts), counts
    assert any("FRAME" in c["paths"] for c in cut["calls"][1:5])
