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
* the quality-7 twins (the fast unit, q_unit_fast, which sets the flag and zeroes the words in code of its own): 44100/128 on the fuzz material runs
  both forms within one call, 44100/320 never the short one, the silence case and the two 32 kHz cases run the short form; and 32000/80 on noise cut
  off at 1.5 kHz, the stream whose bytes depend on the fast unit's zeroing of the words 256..287 (tests/round_skip_cases.py says why);
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
    if name in ("stereo128/fuzz", "stereo128/bursts", "q7/stereo128/fuzz"):
        assert any(h > 0 and f > 0 for h, f in per_call[2:4]), per_call             # inside the 9- or the 17-frame call
    if name == "stereo320/sine":                                                   # (the flush pads the stream with silence: not part of the statement)
        assert all(h == 0 and f > 0 for h, f in per_call[:len(rs.SEQ)]), per_call
    if name == "q7/stereo320/fuzz":                                                # (as above: the stream's own calls)
        assert all(h == 0 for h, f in per_call[:len(rs.SEQ)]) and all(f > 0 for h, f in per_call[:len(rs.SEQ)]), per_call
    if name in ("stereo128/silence", "q7/stereo128/silence"):
        for k in (2, 3):                                                            # the calls that hold the silent stretches
            assert per_call[k][0] > 0 and per_call[k][1] > 0, per_call
    if name in ("stereo32k96/fuzz", "mono32k48/fuzz", "q7/stereo32k96/fuzz", "q7/mono32k48/fuzz"):                             # the cases that fail without the zeroing of words 256..287: the short form must run in them
        assert head > 0 and full > 0, per_call
    if name == "q7/stereo32k80/lownoise":                                          # what makes the zeroing decide bytes: the short form runs, and granules of the batch calls set preflag
        frames = sideinfo.parse(rs.case_stream(name)[3])
        assert all(h > 0 for h, f in per_call[1:4]) and sum(g["preflag"] for fr in frames[1:1 + 2 + 9 + 17] for gg in fr["gr"] for g in gg) >= 20, per_call
    if name.startswith("q7/"):                                                     # every batch call took the fast unit; the one-frame call keeps the general program
        assert [("QUANT_FAST" in r["paths"], "FRAME" in r["paths"]) for r in recs[:len(rs.SEQ)]] == [(False, True)] + [(True, False)] * 3, [r["paths"] for r in recs]
    if c["opts"].get("reservoir") and backend == "hostsim":                        # (one lane: no latency kernels, the chain runs the batch program)
        return
    if c["opts"].get("reservoir"):
        assert any("RESV" in p for r in recs for p in r["paths"]), [r["paths"] for r in recs]


def test_round_skip_wavesim_persistent_forced():
    status, recs, text, fatal = rs.run_child("pair0", "wavesim", 600)
    assert status == 0 and not fatal, (status, text)
    bad = rs.check_records(recs, "pair0")
    assert bad == [], "\n".join(bad)
    two = [r for r in recs if not r.get("done") and r["planned"] in (9, 17) and not r["case"].startswith(("mono", "resv", "q7/"))]
    assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two), [(r["case"], r["paths"]) for r in two]
    q7 = [r for r in recs if not r.get("done") and r["planned"] in (2, 9, 17) and r["case"].startswith("q7/")]
    assert len(q7) == 3 * (len(rs.Q7_TWINS) + 1) and all("QUANT_FAST" in r["paths"] for r in q7), [(r["case"], r["paths"]) for r in q7]


def test_round_skip_case_list():
    """Eleven quality-3 cases, then their six quality-7 twins -- same configuration, material and seed -- and the quality-7 stream of low-passed noise."""
    assert len(rs.CASES) == 11 + 6 + 1 == len({c["name"] for c in rs.CASES}) and not any("quality" in c["opts"] for c in rs.CASES[:11])
    assert [c["name"] for c in rs.CASES[11:]] == ["q7/stereo128/fuzz", "q7/stereo128/silence", "q7/stereo320/fuzz", "q7/lsf64/fuzz", "q7/stereo32k96/fuzz", "q7/mono32k48/fuzz",
                                                  "q7/stereo32k80/lownoise"]
    for c in rs.CASES[11:17]:
        t = rs.case(c["name"][3:])
        assert c["opts"] == {"quality": 7} and t["opts"] == {} and {k: v for k, v in c.items() if k not in ("name", "opts")} == {k: v for k, v in t.items() if k not in ("name", "opts")}


def test_round_skip_material_census():
    cen = sideinfo.census([rs.case_stream(c["name"])[3] for c in rs.CASES])
    assert cen["block_type"][0] > 0 and cen["block_type"][2] > 0 and cen["empty"] > 0 and cen["esc_table"] > 0, cen
    short128 = sideinfo.census([rs.case_stream(n)[3] for n in ("stereo128/fuzz", "stereo128/bursts", "stereo128/silence")])
    assert short128["block_type"][2] > 0 and short128["block_type"][0] > 0, short128
