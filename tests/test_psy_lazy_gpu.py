"""Short-block psychoacoustics only where they are read, on the device (tests/psy_lazy_cases.py; the CPU tier runs every case through both
simulations: tests/test_psy_lazy_cpu.py).  With LAMEJS_PSY_LAZY_MIN_FRAMES=0 -- the hook is read per batch, so everything runs in this
process -- g_psyA<1>, the scans, g_psyA<2> and the lazy g_psyB encode the stereo `bursts` and `sine` cases, the two joint-stereo cases and a
batch of three streams: bytes against the oracle and against the eager launch order, the stream state after every call, and
lhip_debug_read(2) against lhip_debug_read(1) entry by entry.  One stereo `bursts` call of 2048 frames takes the default threshold: bytes
against the oracle, and zeroed short entries in its thresholds show that it ran lazily, while a 40-frame call in the default environment keeps
all 122 entries of every call.  Reads nothing outside the repository tree and oracle/_ref/."""
import numpy as np
import pytest

import psy_lazy_cases as pl
from libs import lib  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pl.GPU_CASES)
def test_gpu_psy_lazy_case(lib, name):
    counts, _ = pl.check_case(lib, name)
    assert len(counts) == 1
    zeroed, computed, needS, needF = counts[0]
    print(name, "zeroed", zeroed, "computed", computed, "needS", needS, "needF", needF)
    expect = pl.case(name)["expect"]
    if expect is not None:
        assert (zeroed + computed, needS, needF) == expect, (name, zeroed, computed, needS, needF)
    assert computed == needS and zeroed > 0 and computed > 0
    if name == "stereo128/bursts":
        assert zeroed >= 40 and computed >= 8, (zeroed, computed)
    if name == "stereo128/sine":
        assert zeroed >= 70, zeroed


def test_gpu_psy_lazy_three_streams_in_one_batch(lib):
    zeroed, computed = pl.check_three_streams(lib)
    assert zeroed > 0 and computed >= 3


def test_gpu_psy_lazy_default_threshold(lib):
    """2048 frame slots and more are a lazy batch without the hook (the default is 6 x CUs, never below 1024); 40 frames are not."""
    name = "stereo128/bursts"
    c = pl.case(name)
    L, R, want = pl.material(name, 1152 * 2048)
    big = pl.encode_calls(lib, c, L, R, [len(L)], None)
    assert big["bytes"] == want
    call = big["calls"][0]
    assert call["frames"] >= 2040 and "SEPARATE" in call["paths"], (call["frames"], sorted(call["paths"]))
    needS, _ = pl.need_flags(call["bt"], [0])
    short_any = pl.u32(call["E"][1:, :, pl.SHORT]).reshape(len(needS) - 1, -1).any(axis=1)
    assert np.array_equal(short_any, needS[1:]), (int(short_any.sum()), int(needS.sum()))
    assert 0 < needS.sum() < len(needS) // 2
    L, R, want = pl.material(name)
    small = pl.encode_calls(lib, c, L, R, [len(L)], None)
    assert small["bytes"] == want
    E = small["calls"][0]["E"]
    assert all(pl.u32(E[g][ch, pl.SHORT]).any() for g in range(1, len(E)) for ch in range(c["ch"]))
