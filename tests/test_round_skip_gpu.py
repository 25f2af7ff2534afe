"""The search without its dead last round of pairs, on the device (tests/round_skip_cases.py; the CPU tier proves the cases and that both
forms run in them: tests/test_round_skip_cpu.py).  One test per environment; each starts tests/tools/round_skip_worker.py as a fresh child
process (LAMEJS_HIP_PAIR_MAX_FRAMES is read once per process) under `timeout -k 10 60` and asserts zero mismatches against the oracle, the
planned frames per call, and the kernels the environment is about: by default a one-frame call takes g_frame (five rounds only) and every
larger two-channel call g_quant_pair; with LAMEJS_HIP_PAIR_MAX_FRAMES=0 the calls of 2, 9 and 17 frames take g_quant and its tail help.  The
quality-7 twins take g_quant_fast in every call of two frames and more, in both environments.

After a child that ended by a signal or a time limit, or whose output holds a HIP error, no further child is started: the later test fails at
once.  Reads nothing outside the repository tree and oracle/_ref/.  A child encodes 18 streams of 30-odd frames: about two seconds with the
interpreter's start and the oracle's side."""
import pytest

import round_skip_cases as rs

pytestmark = pytest.mark.gpu

_fatal = []


def _run(env_name):
    assert not _fatal, f"not started: an earlier child faulted, hung or reported a HIP error ({_fatal[0]})"
    status, recs, text, fatal = rs.run_child(env_name, "gpu", 60)
    if fatal:
        _fatal.append(f"{env_name}: status {status}")
    assert status == 0 and not fatal, (status, text)
    print(env_name, recs[-1])
    bad = rs.check_records(recs, env_name)
    assert bad == [], "\n".join(bad[:40])
    return [r for r in recs if not r.get("done")]


def _two_channel(recs, frames):
    return [r for r in recs if r["planned"] in frames and not r["case"].startswith(("mono", "resv", "q7/"))]


def _fast(recs):
    """The quality-7 twins: g_quant_fast in every batch call, whatever the pair threshold; returns their batch calls."""
    q7 = [r for r in recs if r["planned"] in (2, 9, 17) and r["case"].startswith("q7/")]
    assert len(q7) == 3 * (len(rs.Q7_TWINS) + 1) and all("QUANT_FAST" in r["paths"] and not {"QUANT_PAIR", "QUANT_PERSISTENT"} & set(r["paths"]) for r in q7), [(r["case"], r["paths"]) for r in q7]
    return q7


def test_gpu_round_skip_default():
    recs = _run("default")
    one = [r for r in recs if r["planned"] == 1]
    assert one and all({"FRAME", "FRAME_RESV"} & set(r["paths"]) for r in one), [(r["case"], r["paths"]) for r in one]
    big = _two_channel(recs, (2, 9, 17))
    assert big and all("QUANT_PAIR" in r["paths"] for r in big), [(r["case"], r["paths"]) for r in big]
    mono = [r for r in recs if r["case"].startswith("mono") and r["planned"] in (2, 9, 17)]
    assert mono and all("QUANT_PERSISTENT" in r["paths"] for r in mono)
    _fast(recs)


def test_gpu_round_skip_persistent_forced():
    recs = _run("pair0")
    big = _two_channel(recs, (2, 9, 17))
    assert big and all("QUANT_PERSISTENT" in r["paths"] for r in big), [(r["case"], r["paths"]) for r in big]
    _fast(recs)
