"""calc_noise over the lines its evaluated bands reach, on the device (tests/noise_lines_cases.py; the CPU tier proves which form each case
takes: tests/test_noise_lines_cpu.py).  One test per environment; each starts tests/tools/noise_lines_worker.py as a fresh child process
(LAMEJS_HIP_PAIR_MAX_FRAMES is read once per process) under `timeout -k 10 60` and asserts zero mismatches against the oracle, the planned
frames per call (49 per stream: 1, 2, 9, 17 and 20), and the kernels the environment is about: by default a one-frame call takes g_frame and
every larger two-channel call g_quant_pair, one-channel calls g_quant; with LAMEJS_HIP_PAIR_MAX_FRAMES=0 the two-channel calls of 2 frames and
more take g_quant and its tail help.  The reservoir case takes g_resv_stream.

After a child that ended by a signal or a time limit, or whose output holds a HIP error, no further child is started: the later test fails at
once.  Reads nothing outside the repository tree and oracle/_ref/.  A child encodes nine streams of 49 frames: about two seconds with the
interpreter's start and the oracle's side."""
import pytest

import noise_lines_cases as nl

pytestmark = pytest.mark.gpu

_fatal = []
BATCH = (2, 9, 17, 20)


def _run(env_name):
    assert not _fatal, f"not started: an earlier child faulted, hung or reported a HIP error ({_fatal[0]})"
    status, recs, text, fatal = nl.run_child(env_name, 60)
    if fatal:
        _fatal.append(f"{env_name}: status {status}")
    assert status == 0 and not fatal, (status, text)
    print(env_name, recs[-1])
    bad = nl.check_records(recs, env_name)
    assert bad == [], "\n".join(bad[:40])
    recs = [r for r in recs if not r.get("done")]
    assert {r["case"] for r in recs} == {c["name"] for c in nl.CASES}
    resv = [r for r in recs if r["case"].startswith("resv") and r["planned"] is not None]
    assert resv and all(any("RESV" in p for p in r["paths"]) for r in resv), [(r["case"], r["paths"]) for r in resv]
    return recs


def _two_channel(recs):
    return [r for r in recs if r["planned"] in BATCH and not r["case"].startswith(("mono", "resv"))]


def test_gpu_noise_lines_default():
    recs = _run("default")
    one = [r for r in recs if r["planned"] == 1]
    assert one and all({"FRAME", "FRAME_RESV"} & set(r["paths"]) for r in one), [(r["case"], r["paths"]) for r in one]
    big = _two_channel(recs)
    assert big and all("QUANT_PAIR" in r["paths"] for r in big), [(r["case"], r["paths"]) for r in big]
    mono = [r for r in recs if r["case"].startswith("mono") and r["planned"] in BATCH]
    assert mono and all("QUANT_PERSISTENT" in r["paths"] for r in mono), [(r["case"], r["paths"]) for r in mono]


def test_gpu_noise_lines_persistent_forced():
    recs = _run("pair0")
    big = _two_channel(recs)
    assert big and all("QUANT_PERSISTENT" in r["paths"] for r in big), [(r["case"], r["paths"]) for r in big]
