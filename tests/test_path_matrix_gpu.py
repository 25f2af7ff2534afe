"""Every quantization launch path on every configuration family, on the device (tests/path_matrix_cases.py; the CPU tier proves the cases,
the oracle's expectations, the reader and the bookkeeping first: tests/test_path_matrix_cpu.py).  One test per environment; each starts
tests/tools/path_matrix_worker.py as a fresh child process (the switches are read once per process) under `timeout -k 10`, and asserts

1. zero mismatches against the oracle;
2. every call's path set is the one the expectation table gives for the CU count read at run time, every required (family, path, shape)
   cell was observed and none that the environment makes impossible;
3. (default environment) the material is not trivial: the census of the oracle's bytes.

After a child that ended by a signal or a time limit, or whose output holds a HIP error, no further child is started: the later tests fail
at once.  Reads nothing outside the repository tree and oracle/_ref/.

Time limits, from the children's own wall time measured on an MI355X (10 223 frames each): the worker's encode loop took 2.19 s (default),
2.05 s (pair0), 2.11 s (noframe) and 2.00 s (both); with interpreter start, library load and the oracle's side the tests took 3.5 / 2.5 / 2.7 /
2.5 s.  The limits are 60 s -- more than twenty times that, for a loaded machine -- and 90 s for the default environment, which runs first and
on a fresh checkout also generates the table blobs and builds the oracle (5.1 s measured with the oracle rebuilt)."""
import pytest

import path_matrix_cases as pm
import sideinfo

pytestmark = pytest.mark.gpu

LIMITS = {"default": 90, "pair0": 60, "noframe": 60, "both": 60}
_fatal = []


@pytest.fixture(scope="module")
def num_cus():
    import torch
    assert torch.cuda.is_available()
    n = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert n >= 1
    return n


def _run(env_name, num_cus):
    assert not _fatal, f"not started: an earlier child faulted, hung or reported a HIP error ({_fatal[0]})"
    cs = pm.cases()
    status, recs, text, fatal = pm.run_child(env_name, "gpu", LIMITS[env_name], args=[num_cus])
    if fatal:
        _fatal.append(f"{env_name}: status {status}")
    assert status == 0 and not fatal, (status, text)
    print(env_name, recs[-1])
    bad = pm.check_records(cs, recs, env_name, "gpu", num_cus)
    assert bad == [], "\n".join(bad[:40])
    return recs


def test_gpu_matrix_default(num_cus):
    recs = _run("default", num_cus)
    seen = {p for r in recs for p in r.get("paths", ())}
    assert {"FRAME", "FRAME_RESV", "SEPARATE", "PREP", "PSY4", "QUANT_PAIR", "QUANT_PERSISTENT", "RESV_STREAM_HELPERS", "FIXUP_SINGLE", "FIXUP_COOP", "SMALL_CALL"} <= seen
    assert ("RESV_STREAM_NOHELPERS" in seen) == (pm.RESV_SHAPES["nohelpers"][0] > num_cus)
    # the material (the oracle's bytes alone)
    cs = pm.cases()
    joint = sideinfo.census([st[4] for c in cs if c["kind"] == "joint" for st in pm.case_streams(c)])
    for fam in pm.TWO_CHANNEL:
        cen = sideinfo.census([st[4] for c in cs if c["kind"] == "stereo" and c["family"] == fam for st in pm.case_streams(c)])
        assert pm.census_ok(fam, cen, joint if fam == "mpeg1" else None) == [], fam


def test_gpu_matrix_persistent_forced(num_cus):
    """LAMEJS_HIP_PAIR_MAX_FRAMES=0: every two-channel batch through g_quant and tail_help -- every two-channel configuration, joint,
    protect, Float32 interleaved with gains, at every shape >= 2."""
    recs = _run("pair0", num_cus)
    two = [r for r in recs if r.get("kind") in pm.TWO_OUT and "paths" in r]
    assert two and all("QUANT_PERSISTENT" in r["paths"] for r in two if "SEPARATE" in r["paths"])
    assert {r["frames"] for r in two if "QUANT_PERSISTENT" in r["paths"]} >= set(pm.SHAPES) - {1}


def test_gpu_matrix_separate_forced(num_cus):
    recs = _run("noframe", num_cus)
    assert not any({"FRAME", "FRAME_RESV"} & set(r.get("paths", ())) for r in recs)


def test_gpu_matrix_both_forced(num_cus):
    recs = _run("both", num_cus)
    assert not any({"FRAME", "FRAME_RESV", "QUANT_PAIR"} & set(r.get("paths", ())) for r in recs)
