"""The search without its dead last round of pairs, CPU tier: the cases of tests/round_skip_cases.py through the one-lane and the 64-lane
simulations, byte for byte against the oracle, with the simulations' two counters (evaluations made without / with the last round,
lhip_debug_read(10)) proving that the cases are not trivial:

* 44100/128 stereo on the fuzz material and on `bursts`: both forms run within one call, the 9- or the 17-frame one;
* 44100/320 stereo `sine`: no evaluation of the stream's own calls takes the short form (every long-block granule-channel keeps lines at or
  above 518; the flush, which pads with silence, is not part of the statement);
* noise with stretches of digital silence: the short form's counter rises over the calls that hold the stretches.  A granule-channel of pure
  digital silence makes no evaluation at all (init_xrpow finds no energy), so what rises it is the long blocks behind the noise's onset --
  the units that would inherit a short block's words 256..287 -- and the full form's counter must rise there too (the onset itself);
* 32000/96 stereo and 32000/48 mono, where band 20 covers the lines 448..549: the short form runs, and with the simulations' poison in the words
  256..287 at every granule-channel's entry these two streams differ from the oracle if q_unit does not zero them (tests/round_skip_cases.py);
* the census of the oracle's bytes (tests/sideinfo.py) shows long and short blocks, an empty granule-channel and an ESC table.

The 64-lane simulation also runs the cases with LAMEJS_HIP_PAIR_MAX_FRAMES=0 in a child process (tests/tools/round_skip_worker.py): its
nine-frame call takes the pair program by default and the eight-wave workgroup with the tail help then."""
import pytest

import round_skip_cases as rs
import sideinfo
from libs import sim_library

BACKENDS = ("hostsim", "wavesim")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [c["name"] for c in rs.CASES])
def test_round_skip_sim(backend, name):
    lib = sim_library(backend)
    c = rs.case(name)
    marks = []
    recs = rs.encode_case(lib, c, before_call=lambda k: marks.append(rs.round_counts(lib)))
    bad = rs.check_records(recs + [{"done": True, "cases": len(rs.CASES)}], backend)
    assert bad == [], "\n".join(bad)
    assert [r["frames"] for r in recs[:len(rs.SEQ)]] == list(rs.SEQ)
    per_call = [(b[0] - a[0], b[1] - a[1]) for a, b in zip(marks, marks[1:])]      # (short form, full form) evaluations of call k
    print(name, backend, per_call)
    head, full = sum(h for h, _ in per_call), sum(f for _, f in per_call)
    assert head + full > 0
    if name in ("stereo128/fuzz", "stereo128/bursts"):
        assert any(h > 0 and f > 0 for h, f in per_call[2:4]), per_call             # inside the 9- or the 17-frame call
    if name == "stereo320/sine":                                                   # (the flush pads the stream with silence: not part of the statement)
        assert all(h == 0 and f > 0 for h, f in per_call[:len(rs.SEQ)]), per_call
    if name == "stereo128/silence":
        for k in (2, 3):                                                            # the calls that hold the silent stretches
            assert per_call[k][0] > 0 and per_call[k][1] > 0, per_call
    if name in ("stereo32k96/fuzz", "mono32k48/fuzz"):                             # the cases that fail without the zeroing of words 256..287: the short form must run in them
        assert head > 0 and full > 0, per_call
    if c["opts"].get("reservoir") and backend == "hostsim":                        # (one lane: no latency kernels, the chain runs the batch program)
        return
    if c["opts"].get("reservoir"):
        assert any("RESV" in p for r in recs for p in r["paths"]), [r["paths"] for r in recs]


def test_round_skip_wavesim_persistent_forced():
    status, recs, text, fatal = rs.run_child("pair0", "wavesim", 600)
    assert status == 0 and not fatal, (status, text)
    bad = rs.check_records(recs, "pair0")
    assert bad == [], "\n".join(bad)
    two = [r for r in recs if not r.get("done") and r["planned"] in (9, 17) and not r["case"].startswith(("mono", "resv"))]
    assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two), [(r["case"], r["paths"]) for r in two]


def test_round_skip_material_census():
    cen = sideinfo.census([rs.case_stream(c["name"])[3] for c in rs.CASES])
    assert cen["block_type"][0] > 0 and cen["block_type"][2] > 0 and cen["empty"] > 0 and cen["esc_table"] > 0, cen
    short128 = sideinfo.census([rs.case_stream(n)[3] for n in ("stereo128/fuzz", "stereo128/bursts", "stereo128/silence")])
    assert short128["block_type"][2] > 0 and short128["block_type"][0] > 0, short128
