"""calc_noise over the lines its evaluated bands reach, CPU tier: the cases of tests/noise_lines_cases.py (24 frames each: calls completing 1, 2, 9
and 12 frames, then the flush) through the 64-lane wave simulation, byte for byte against the oracle, with the simulation's counter of calc_noise
calls made with 7, with 9 and with 3 lines per lane (lhip_debug_read(12)) proving which forms a case takes:

* 44100/128 stereo and mono on `sine` and `bursts`, 48000/192 stereo, 44100/128 with the bit reservoir: every full call in the 7-line form, none in the 9-line one;
* 32000/64 mono (sfb_l[21] = 550) and 22050/64 stereo (MPEG-2, sfb_l[21] = 522): every full call in the 9-line form, none in the 7-line one;
* every case also makes calls in the short window (3 lines per lane over lines 0..191: all fresh bands end at or below line 192);
* the form is the rule of lhip_tables.h applied to the case's own table blob (noise_lines_cases.expected_nln);
* `bursts` brings short blocks (the census of the oracle's bytes), whose last evaluated line is 407 at 44.1 kHz;
* 44100/128 stereo `sine` reaches band 20 (lines 342..417, through lane 59 of the 7-line layout): the side records of its 12-frame call
  (lhip_debug_read(4)) hold long-block granules whose scalefactor of band 20 is above zero -- the outer loop found that band distorted and
  amplified it -- and the bytes those scalefactors went into equal the oracle's."""
import ctypes

import numpy as np
import pytest

import noise_lines_cases as nl
import sideinfo
from libs import sim_library
from stage_taps import GRSIDE


def _band20_amplified(lib, c, frames):
    """Long-block granule-channels of the last batch whose kept scalefactor of band 20 is above zero."""
    a = np.empty(frames * 2 * c["ch"], dtype=GRSIDE)
    assert lib.lhip_debug_read(4, a.ctypes.data_as(ctypes.c_void_p), a.nbytes) == a.nbytes
    return int(sum(1 for s in a if s["active"] and s["block_type"] != 2 and s["scalefac"][20] > 0))


@pytest.mark.parametrize("name", [c["name"] for c in nl.CASES])
def test_noise_lines_wavesim(name):
    lib = sim_library("wavesim")
    c = nl.case(name)
    want_nln = nl.expected_nln(c)
    assert want_nln == (7 if name in nl.SEVEN else 9) and (name in nl.SEVEN) != (name in nl.NINE), (name, nl.band_borders(c))
    band20 = []

    def after_call(k, enc):
        if name == "stereo128/sine" and k == 3:
            band20.append(_band20_amplified(lib, c, nl.SEQ_CPU[3]))

    before = nl.line_counts(lib)
    recs = nl.encode_case(lib, c, nl.SEQ_CPU, after_call)
    n7, n9, n3 = (b - a for a, b in zip(before, nl.line_counts(lib)))
    print(name, "calc_noise calls with 7 / 9 / 3 lines per lane:", n7, n9, n3, "borders", nl.band_borders(c), "band 20 amplified in", band20)
    bad = nl.check_records(recs + [{"done": True, "cases": 1}], "wavesim", ncases=1)
    assert bad == [], "\n".join(bad)
    assert [r["frames"] for r in recs[:len(nl.SEQ_CPU)]] == list(nl.SEQ_CPU)
    if want_nln == 7:
        assert n7 > 0 and n9 == 0, (n7, n9)
    else:
        assert n9 > 0 and n7 == 0, (n7, n9)
    assert n3 > 0, (n7, n9, n3)                      # the short window runs in every case, beside the full form
    if name == "stereo128/sine":
        assert band20 and band20[0] > 0, band20
    if c["opts"].get("reservoir"):
        assert any("RESV" in p for r in recs for p in r["paths"]), [r["paths"] for r in recs]
    else:
        assert "FRAME" in recs[0]["paths"], recs[0]["paths"]


def test_noise_lines_borders():
    """The borders the case list is built on, from the blobs themselves: 44.1 and 48 kHz fit 448 lines, 32 and 22.05 kHz do not."""
    got = {c["name"]: nl.band_borders(c) for c in nl.CASES}
    assert got["stereo128/sine"] == (418, 408) and got["stereo48k192/sine"] == (384, 378), got
    assert got["mono32k64/sine"][0] == 550 and got["lsf64/sine"][0] > 448, got


def test_noise_lines_material_census():
    for name in ("stereo128/bursts", "mono128/bursts", "stereo48k192/bursts"):
        cen = sideinfo.census([nl.case_stream(name, nl.SEQ_CPU)[3]])
        assert cen["block_type"][2] > 0 and cen["block_type"][0] > 0, (name, cen)
